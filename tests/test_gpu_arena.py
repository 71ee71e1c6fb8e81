"""Arena on the GPU: the four hive_arena_* kernels against restatements in torch / Python, mcts.ArenaSearch against the
single-network search on the games each network owns, and arena.Arena end to end (self-consistency, independence from the
batch, the reference's recorded games, the CPU oracle)."""
import ctypes
import itertools

import pytest
import torch

from test_arena_host import opening_action


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from hive_alphazero_amd import _lib as m
    return m.load(), m.check


def cheap_evaluator(planes):
    """A position's (p, v) from integer hashes of its planes: exact, so the same bits in any batch at any row."""
    B = planes.shape[0]
    x = planes.reshape(B, 144, 56).to(torch.int64)
    dev = planes.device
    cell = (x * (torch.arange(56, device=dev) * 37 % 101 + 1)).sum(2)                      # [B,144]
    h = (cell * (torch.arange(144, device=dev) * 53 % 97 + 1)).sum(1, keepdim=True)       # [B,1]
    j = torch.arange(1584, device=dev).view(1, -1)
    mix = (h * (2 * j + 1) + cell[:, torch.arange(1584, device=dev) % 144] * 7919) % 1009
    p = (mix.float() + 1.0) / (1584.0 * 505.0)
    v = ((h.view(-1) * 31) % 2001).float() / 1000.0 - 1.0
    return p, v * 0.9


@pytest.fixture(scope="module")
def nets():
    """ChessNet seeded 0 (A), seeded 1 (B) and seeded 0 again (A2: a second evaluator of A's weights)."""
    from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
    out = []
    for seed in (0, 1, 0):
        torch.manual_seed(seed)
        out.append(InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16))
    return out


def _roots(n, seed, games, skip):
    """n positions `skip / games` plies and more into random playouts (both turn parities) -> (boards, history)."""
    from hive_alphazero_amd import batch, playout
    boards = playout.random_positions(n + skip, seed=seed, games=games)[skip:].contiguous()
    B = batch.BoardBatch(n)
    B.import_state(boards)
    rb, rh = B.export_state()
    B.close()
    return rb, rh


# ------------------------------------------------------------------------------------------ 1. split / join
@pytest.mark.gpu
@pytest.mark.parametrize("games,slots", [(1, 1), (63, 1), (65, 3), (1000, 4)])
def test_split_and_join_equal_torch_where(games, slots):
    L, check = _lib()
    gen = torch.Generator(device="cuda").manual_seed(games * 10 + slots)
    n = games * slots
    roots = torch.zeros((games, 64), dtype=torch.uint8, device="cuda")
    roots[:, 33] = torch.randint(1, 55, (games,), device="cuda", generator=gen).to(torch.uint8)
    a_white = torch.randint(0, 2, (games,), device="cuda", generator=gen).to(torch.int8)
    need = torch.randint(0, 2, (n,), device="cuda", generator=gen).to(torch.int8)
    owner_a = ((a_white != 0) == (roots[:, 33] % 2 == 1)).repeat(slots)                    # row r -> game r % games
    for nd in (need, None):
        need_a = torch.full((n,), 7, dtype=torch.int8, device="cuda")
        need_b = torch.full((n,), 7, dtype=torch.int8, device="cuda")
        rows = torch.tensor([5, 11], dtype=torch.int64, device="cuda")
        check(L.hive_arena_split_launch(_p(roots), _p(a_white), _p(nd), games, slots, _p(need_a), _p(need_b),
                                        ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(rows.data_ptr() + 8), _stream()))
        want = nd if nd is not None else torch.ones_like(need)
        zero = torch.zeros_like(want)
        want_a, want_b = torch.where(owner_a, want, zero), torch.where(owner_a, zero, want)
        assert torch.equal(need_a, want_a) and torch.equal(need_b, want_b)
        assert rows.tolist() == [5 + int(want_a.sum()), 11 + int(want_b.sum())]
        # counters are optional
        check(L.hive_arena_split_launch(_p(roots), _p(a_white), _p(nd), games, slots, _p(need_a), _p(need_b), None, None, _stream()))
        assert torch.equal(need_a, want_a) and torch.equal(need_b, want_b)
    p_a = torch.rand((n, 1584), device="cuda", generator=gen)
    p_b = torch.rand((n, 1584), device="cuda", generator=gen)
    v_a = torch.rand((n,), device="cuda", generator=gen)
    v_b = torch.rand((n,), device="cuda", generator=gen)
    want_p, want_v = torch.where(owner_a.view(-1, 1), p_a, p_b), torch.where(owner_a, v_a, v_b)
    pb0, vb0 = p_b.clone(), v_b.clone()
    check(L.hive_arena_join_launch(_p(roots), _p(a_white), games, slots, _p(p_a), _p(v_a), _p(p_b), _p(v_b), _stream()))
    assert torch.equal(p_a, want_p) and torch.equal(v_a, want_v)
    assert torch.equal(p_b, pb0) and torch.equal(v_b, vb0)


# ------------------------------------------------------------------------------------------ 2. score
@pytest.mark.gpu
def test_score_kernel_on_every_combination():
    L, check = _lib()
    combos = list(itertools.product((0, 1), (0, 1, 2), (0, 1), (54, 55), (0, 1)))          # a_white, winner, over, turn, active
    combos = combos * 3                                                                     # more than one wave
    n = len(combos)
    col = lambda k, dt: torch.tensor([c[k] for c in combos], dtype=dt, device="cuda")
    a_white, winner, over, turn, active = col(0, torch.int8), col(1, torch.int8), col(2, torch.int8), col(3, torch.uint8), col(4, torch.int8)
    boards = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    boards[:, 33] = turn
    want, tally = [], [0] * 8
    for aw, w, ov, t, act in combos:
        res = 0
        if act and ov:
            if w == 1:
                res = 1 if aw else 2
                tally[0 if aw else 2] += 1
            elif w == 2:
                res = 2 if aw else 1
                tally[3 if aw else 1] += 1
            else:
                res = 3
                tally[4] += 1
        elif act and t >= 55:
            res = 4
            tally[5] += 1
        if res:
            tally[6] += 1
            tally[7] += t
        want.append(res)
    result = torch.full((n,), 9, dtype=torch.int8, device="cuda")
    got = torch.tensor([100, 0, 0, 0, 0, 0, 0, 1000], dtype=torch.int32, device="cuda")      # the tally is added to
    check(L.hive_arena_score_launch(_p(boards), _p(over), _p(winner), _p(active), _p(a_white), n, 55, _p(result), _p(got), _stream()))
    assert result.tolist() == want
    tally[0] += 100
    tally[7] += 1000
    assert got.tolist() == tally
    assert set(want) == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------ 3. opening
@pytest.mark.gpu
def test_opening_draw_equals_the_python_mirror():
    from hive_alphazero_amd import batch, playout
    L, check = _lib()
    n, seed = 37, 0xC0FFEE123456789
    boards = playout.random_positions(n, seed=31)
    boards[1] = boards[20]                                       # two boards with the same position ...
    _, count, lst = batch.movegen(boards, want_list=True)
    pair = torch.tensor([(i * 7919 + 3) % 1000 for i in range(n)], dtype=torch.int64, device="cuda")
    pair[1] = pair[20]                                           # ... and the same pair
    turns = [1 + i % 6 for i in range(n)]
    turns[1] = turns[20] = 3
    boards[:, 33] = torch.tensor(turns, dtype=torch.uint8, device="cuda")
    count[8] = 0                                                 # turn 3, no legal move: a pass
    active = torch.ones((n,), dtype=torch.int8, device="cuda")
    active[12] = 0                                               # turn 1, idle slot
    action = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    check(L.hive_arena_opening_launch(_p(boards), _p(count), _p(lst), _p(pair), _p(active), n, ctypes.c_uint64(seed), 4,
                                      _p(action), _stream()))
    got, cnt, ids, pairs = action.tolist(), count.tolist(), lst.cpu().tolist(), pair.tolist()
    for i in range(n):
        if turns[i] > 4 or i == 12:
            assert got[i] == -7, i
        else:
            assert got[i] == opening_action(seed, pairs[i], turns[i], ids[i][:cnt[i]]), i
    assert got[8] == -1 and turns[8] == 3
    assert got[1] == got[20] >= 0
    assert len({got[i] for i in range(n) if turns[i] <= 4}) > 4
    # active == NULL: every game
    check(L.hive_arena_opening_launch(_p(boards), _p(count), _p(lst), _p(pair), None, n, ctypes.c_uint64(seed), 4, _p(action), _stream()))
    assert action[12].item() == opening_action(seed, pairs[12], turns[12], ids[12][:cnt[12]])


# ------------------------------------------------------------------------------------------ 4. / 5. ownership
def _ownership(nets, G, sims, slots_list, eps_list, roots_seed, playout_games, skip):
    from hive_alphazero_amd import mcts
    A, B, _ = nets
    rb, rh = _roots(G, roots_seed, playout_games, skip)
    turn = rb[:, 33]
    assert bool((turn % 2 == 1).any()) and bool((turn % 2 == 0).any()) and int(turn.min()) >= 3
    gen = torch.Generator(device="cuda").manual_seed(G)
    a_white = torch.randint(0, 2, (G,), device="cuda", generator=gen).to(torch.int8)
    own_a = (a_white != 0) == (turn % 2 == 1)
    assert 0 < int(own_a.sum()) < G
    ids = torch.arange(G, device="cuda") * 3 + 1000
    for slots, eps in itertools.product(slots_list, eps_list):
        out = {}
        for name in ("a", "b", "arena"):
            if name == "arena":
                ts = mcts.ArenaSearch(G, sims, A, B, a_white, slots=slots, seed=9, noise_eps=eps)
                assert ts._nets[0]["share"] and ts._nets[1]["share"]
            else:
                ts = mcts.TreeSearch(G, sims, A if name == "a" else B, slots=slots, seed=9, noise_eps=eps)
                assert ts.share_equal_leaves
            ts.set_game_ids(ids)
            action, policy, sum_n = ts.search(rb, rh)
            rows = ts.rows_evaluated() if name == "arena" else None
            out[name] = (action.clone(), policy.clone(), sum_n.clone(), int(ts.evals_run.item()), rows, ts.evals_launched)
            ts.close()
        for name, own in (("a", own_a), ("b", ~own_a)):
            for x, y in zip(out["arena"][:3], out[name][:3]):
                assert torch.equal(x[own], y[own]), (name, slots, eps)
        ra, rb_ = out["arena"][4]
        print(f"G {G} slots {slots} eps {eps}: rows A {ra} (single {out['a'][3]}), B {rb_} (single {out['b'][3]}), "
              f"launched {out['arena'][5]}")
        assert ra + rb_ == out["arena"][3] and out["arena"][5] == out["a"][5]
        assert 0 < ra <= out["a"][3] and 0 < rb_ <= out["b"][3]
        assert ra + rb_ <= out["a"][3] + out["b"][3] and ra + rb_ <= out["arena"][5]
        assert bool((out["a"][1] != out["b"][1]).any())          # the two networks do search differently


@pytest.mark.gpu
def test_each_side_is_searched_by_its_own_network(nets):
    _ownership(nets, G=64, sims=8, slots_list=(1, 4), eps_list=(0.25, 0.0), roots_seed=41, playout_games=8, skip=16)


@pytest.mark.gpu
def test_ownership_through_the_72_tile_tower(nets):
    assert nets[0]._tower_form(448) == 72 and nets[0].accepts_need and nets[0].accepts_rep
    _ownership(nets, G=448, sims=3, slots_list=(1,), eps_list=(0.25,), roots_seed=43, playout_games=32, skip=64)


@pytest.mark.gpu
def test_arena_search_refuses_the_reuse_store():
    from hive_alphazero_amd import mcts
    a_white = torch.zeros((4,), dtype=torch.int8, device="cuda")
    with pytest.raises(ValueError):
        mcts.ArenaSearch(4, 2, cheap_evaluator, cheap_evaluator, a_white, reuse_store=1 << 12)


# ------------------------------------------------------------------------------------------ 6. A against itself
@pytest.mark.gpu
def test_second_evaluator_of_the_same_weights_plays_the_same_games(nets):
    from hive_alphazero_amd.arena import Arena
    A, _, A2 = nets
    moves = []
    for other in (A2, A):
        ar = Arena(A, other, pairs=16, sims=6, seed=3)
        for _ in range(10):
            ar.play_ply()
        assert ar.illegal_count() == 0
        moves.append(ar.moves.cpu())
        ar.close()
    assert torch.equal(moves[0], moves[1])
    m = moves[0]
    assert bool((m[:, :4] >= 0).all()) and bool((m[:, 4:10] >= -1).all())
    assert torch.equal(m[0::2, :4], m[1::2, :4])                 # both games of a pair share their opening
    assert len({tuple(r) for r in m[:, :4].tolist()}) > 4        # and the pairs' openings differ


# ------------------------------------------------------------------------------------------ 7. batch independence
@pytest.mark.gpu
def test_games_do_not_depend_on_the_games_in_flight():
    from hive_alphazero_amd.arena import Arena
    out = []
    for inflight in (32, 8):
        ar = Arena(cheap_evaluator, cheap_evaluator, pairs=16, sims=6, games_in_flight=inflight, seed=11)
        res = ar.run()
        assert ar.illegal_count() == 0 and res.games == 32 and sorted(ar.games) == list(range(32))
        assert ar.rows_evaluated()[0] == ar.rows_evaluated()[1] > 0          # stubs see the whole batch
        out.append((ar.games, res.as_dict()))
        ar.close()
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1]
    for code, moves in out[0][0].values():
        assert code in (1, 2, 3, 4) and 0 < len(moves) <= 54


# ------------------------------------------------------------------------------------------ 8. the reference's games
@pytest.mark.gpu
def test_scoring_of_the_reference_games(golden_games):
    from hive_alphazero_amd.arena import A_WIN, B_WIN, CAP, DRAW, Arena
    games = golden_games[:60]                                    # games_full.json.gz
    ends = [(bool(g["plies"][-1]["over"]), int(g["plies"][-1]["win"])) for g in games]
    assert sum(o and w == 1 for o, w in ends) == 7 and sum(o and w == 2 for o, w in ends) == 3
    assert sum((not o) and g["plies"][-1]["t"] == 55 for (o, _), g in zip(ends, games)) == 50
    ar = Arena(cheap_evaluator, cheap_evaluator, pairs=30, sims=2, games_in_flight=60, seed=1)
    ply = 0
    while ar.running():
        forced = []
        for g in games:
            a = g["plies"][ply]["a"] if ply < len(g["plies"]) - 1 else -2
            forced.append(-1 if a is None else int(a))
        ar.play_ply(torch.tensor(forced, dtype=torch.int32))
        ply += 1
        assert ply <= 60
    assert ar.illegal_count() == 0
    want, tally = {}, [0] * 8
    for s, ((over, win), g) in enumerate(zip(ends, games)):
        a_white = s % 2 == 0                                     # slot s played game id s: pair s // 2, A white in the even one
        if over and win == 1:
            want[s] = A_WIN if a_white else B_WIN
            tally[0 if a_white else 2] += 1
        elif over and win == 2:
            want[s] = B_WIN if a_white else A_WIN
            tally[3 if a_white else 1] += 1
        elif over:
            want[s] = DRAW
            tally[4] += 1
        else:
            want[s] = CAP
            tally[5] += 1
        tally[6] += 1
        tally[7] += g["plies"][-1]["t"]
    assert ar.results == want
    assert ar.tally.tolist() == tally
    for s, g in enumerate(games):
        assert ar.games[s] == (want[s], [-1 if p["a"] is None else int(p["a"]) for p in g["plies"][:-1]]), s
    res = ar.result()
    assert (res.wins + res.losses, res.draws, res.caps, res.games) == (10, 0, 50, 60) and len(res.pair_scores) == 30
    ar.close()


# ------------------------------------------------------------------------------------------ 9. whole games vs the oracle
@pytest.mark.gpu
def test_whole_match_replays_on_the_oracle(nets):
    from hive_alphazero_amd.arena import A_WIN, B_WIN, CAP, DRAW, Arena, game_pair
    from oracle_env import PIECE_BLACK, PIECE_WHITE, OracleGamePlay
    A, B, _ = nets
    ar = Arena(A, B, pairs=8, sims=4, seed=5)
    res = ar.run()
    assert ar.illegal_count() == 0 and res.games == 16 and sorted(ar.games) == list(range(16))
    for gid, (code, moves) in ar.games.items():
        pair, a_white = game_pair(gid)
        g = OracleGamePlay()
        for a in moves:
            assert not g.game_is_over()
            legal = g.actions()
            assert (a in legal) if legal else a == -1, (gid, a)
            g.move(a)
        over = g.game_is_over()
        if over and g.state.winner == PIECE_WHITE:
            want = A_WIN if a_white else B_WIN
        elif over and g.state.winner == PIECE_BLACK:
            want = B_WIN if a_white else A_WIN
        elif over:
            want = DRAW
        else:
            assert g.turn() == 55
            want = CAP
        assert code == want, gid
        w, b = ar.games[2 * pair][1], ar.games[2 * pair + 1][1]
        assert w[:4] == b[:4]
    assert res.wins + res.losses + res.draws + res.caps == 16
    a_rows, b_rows = ar.rows_evaluated()
    assert a_rows > 0 and b_rows > 0
    print(res)
    ar.close()
