"""Proven wins and losses below the root on the GPU (hive_search_set_solver): the finishing move a tree holds is played, the
search against the sequential statement over whole trees, soundness of every proof against the CPU oracle, the `where` mask
bit for bit, and the option under budgets, per-game clocks, kept trees, the unread-row flags and the arena."""
import json
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

import solver_cases as S
from hive_alphazero_amd import mcts
from test_gpu_gumbel import (_host_stub_evaluator, _ids, _outputs, _same_rows, _same_tree, other_evaluator, stub_evaluator)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 55
SEED = 11
# decisive_games(333, 11), one ply before the end: win-in-one roots at which the plain sequential search of 40 simulations
# answers another move while the solver search expands the finishing edge (chosen on the CPU, tests/test_solver_host.py)
SIMS_WIN = 40
WIN_IN_ONE = [15, 19, 45, 53, 137, 159, 168, 189, 228, 332]
# (game, plies before the end) of decisive_games(57, 11) for the mirror, plus the recorded forced loss
SIMS_MIRROR = 48
MIRROR = [(40, 2), (41, 3), (46, 3), (52, 2), (56, 2), (15, 1), (53, 1)]


def _i8(x):
    return torch.tensor(x, dtype=torch.int8, device="cuda")


@pytest.fixture(scope="module")
def games():
    return S.decisive_games(max(WIN_IN_ONE) + 1, SEED)


def _lost_game():
    with open(os.path.join(ROOT, "tests", "golden", "solver_lost_game.json")) as f:
        rec = json.load(f)
    return rec["moves"][:rec["lost_after_plies"]]


def _roots(move_lists):
    """(boards, history) after each move list, played from the opening position on the GPU env."""
    from hive_alphazero_amd import batch
    n = len(move_lists)
    B = batch.BoardBatch(n)
    for ply in range(max(len(m) for m in move_lists)):
        B.step([int(m[ply]) if ply < len(m) else -2 for m in move_lists])
    assert B.illegal_count() == 0
    rb, rh = B.export_state()
    B.close()
    return rb, rh


def _search(G, sims, solver=True, evaluator=_host_stub_evaluator, seed=9, noise_eps=0.0, **kw):
    ts = mcts.TreeSearch(G, sims, evaluator, plane_dtype=torch.float32, seed=seed, noise_eps=noise_eps, solver=solver, **kw)
    ts.set_game_ids(_ids(G))
    return ts


def _node_envs(tree, env):
    """{node: oracle env of its position}, walking the exported tree from the root by its own edges' actions."""
    envs, todo = {0: env}, [0]
    while todo:
        k = todo.pop()
        for e in range(int(tree["nedge"][k])):
            c = int(tree["child"][k, e])
            if c >= 0 and c not in envs:
                nxt = deepcopy(envs[k])
                nxt.move(int(tree["act"][k, e]))
                envs[c] = nxt
                todo.append(c)
    return envs


# ------------------------------------------------------------------------------------------ 4. fails without the feature
def test_the_finishing_move_in_the_tree_is_played(games):
    """Ten win-in-one roots, 40 simulations, no root noise, the host stub evaluator: the plain search answers another move
    (on the CPU and here), the solver search expands the finishing edge, proves the root +2 and plays it.  The policy row
    is the visit distribution of the simulations before the proof: the plain search of sum_n + 1 simulations, bit for bit."""
    G = len(WIN_IN_ONE)
    prefixes = [games[k][0][:-1] for k in WIN_IN_ONE]
    finishing = [S.finishing_moves(S.env_after(m)) for m in prefixes]
    assert all(games[k][0][-1] in f for k, f in zip(WIN_IN_ONE, finishing))
    rb, rh = _roots(prefixes)
    plain = _search(G, SIMS_WIN, solver=False)
    plain_out = _outputs(plain, plain.search(rb, rh))
    ts = _search(G, SIMS_WIN)
    action, policy, sum_n = [x.clone() for x in ts.search(rb, rh)]
    status, stats = ts.root_status().cpu().numpy(), ts.solver_stats().cpu().numpy()
    print("plain", plain_out[0].tolist(), "solver", action.tolist(), "sum_n", sum_n.tolist(), "stats", stats.tolist())
    assert status.dtype == np.int8 and status.tolist() == [2] * G
    for g in range(G):
        assert int(action[g]) in finishing[g] and int(plain_out[0][g]) not in finishing[g], g
        node, edge = ts.node_status(g)
        tree = ts.export_tree(g)
        e = tree["act"][0, :int(tree["nedge"][0])].tolist().index(int(action[g]))
        assert node[0] == 2 and edge[0, e] == 2 and tree["n_visits"][0, e] == 1
        assert node[int(tree["child"][0, e])] == -1 and tree["term"][int(tree["child"][0, e])]
    assert (stats[:, 3] == 1).all() and (stats[:, 1] == 1).all() and (stats[:, 2] == 0).all()
    # the simulations after the proof ended at the root and left no visit
    assert (stats[:, 0] == SIMS_WIN - 1 - sum_n.cpu().numpy()).all() and (sum_n <= SIMS_WIN - 1).all() and (sum_n < SIMS_WIN - 1).sum() >= 8
    short = _search(G, SIMS_WIN, solver=False)
    short_out = short.search(rb, rh, budgets=(sum_n + 1).to(torch.int32))
    assert torch.equal(short_out[2], sum_n) and torch.equal(short_out[1].view(torch.int32), policy.view(torch.int32))
    for ts_ in (plain, ts, short):
        ts_.close()


# ------------------------------------------------------------------------------------------ 5. / 6. the mirror, soundness
@pytest.fixture(scope="module")
def mirror(games):
    """Eight searches of 48 simulations from positions one to three plies before the end, on the GPU and by the sequential
    player: computed once, left unchanged."""
    prefixes = [games[k][0][:-cut] for k, cut in MIRROR] + [_lost_game()]
    G = len(prefixes)
    rb, rh = _roots(prefixes)
    ts = _search(G, SIMS_MIRROR)
    out = [x.clone() for x in ts.search(rb, rh)]
    cases = []
    for g in range(G):
        env = S.env_after(prefixes[g])
        player, move, policy, visits = S.run_player(env, SIMS_MIRROR, True)
        node, edge = ts.node_status(g)
        cases.append({"env": env, "player": player, "move": move, "policy": policy, "visits": visits,
                      "tree": ts.export_tree(g), "node": node, "edge": edge})
    stats = ts.solver_stats().cpu().numpy()
    ts.close()
    return {"out": out, "cases": cases, "stats": stats}


def test_whole_trees_match_the_sequential_statement(mirror):
    """GPU tree and player table walked together from the root by action id: every node status, edge status and N equal,
    W within 6e-8 N (1 + N) -- the player sums float64 values of float64 network outputs, the GPU fp32 ones: each of the N
    terms differs by at most 2^-24 relative and each of the N additions rounds a sum of magnitude at most N at 2^-24 --
    and the action, the policy and the counters the same.
    The inputs, counted on the CPU over the player's eight tables: 9 proven-win entries, 6 edges with status -3, 2
    proven-loss entries by the all-edges rule (the forced pass of the recorded game and the position two plies on)."""
    import hive_alphazero_amd.solo_play as sp
    wins = losses = minus3 = 0
    for c in mirror["cases"]:
        for entry in c["player"]._table.values():
            wins += entry.status > 0
            losses += entry.status < 0
            minus3 += 0 if entry.es is None else int((entry.es == -3).sum())
    print(f"proven-win entries {wins}, proven-loss entries {losses}, edges at -3 {minus3}")
    assert wins >= 8 and minus3 >= 4 and losses >= 1
    action, policy, sum_n = mirror["out"]
    for g, c in enumerate(mirror["cases"]):
        tree, node, edge, player = c["tree"], c["node"], c["edge"], c["player"]
        assert int(action[g]) == c["move"] and int(sum_n[g]) == c["visits"], g
        if player._table[c["env"].state_key].moves != [-1]:            # (a forced pass writes no policy entry on the GPU)
            assert np.abs(policy[g].cpu().numpy().astype(np.float64) - c["policy"]).max() < 1e-6, g
        else:
            assert not policy[g].any() and c["move"] == -1
        assert mirror["stats"][g].tolist() == player.solver_stats, g
        todo, seen = [(0, deepcopy(c["env"]))], {0}
        while todo:
            k, env = todo.pop()
            entry = player._table[env.state_key]
            assert int(node[k]) == entry.status, (g, k)
            ne = int(tree["nedge"][k])
            if entry.moves is None:
                assert not tree["n_visits"][k, :ne].any() and not edge[k, :ne].any(), (g, k)
                continue
            assert tree["act"][k, :ne].tolist() == list(entry.moves), (g, k)
            assert tree["n_visits"][k, :ne].tolist() == entry.n.tolist(), (g, k)
            assert edge[k, :ne].tolist() == entry.es.tolist(), (g, k)
            n = entry.n.astype(np.float64)
            assert (np.abs(tree["w"][k, :ne].astype(np.float64) - entry.w) <= 6e-8 * n * (1 + n) + 1e-12).all(), (g, k)
            for e in range(ne):
                ch = int(tree["child"][k, e])
                assert ch >= -1
                if ch < 0:
                    assert edge[k, e] == 0                              # an edge that is not expanded proves nothing
                    continue
                if ch in seen:
                    continue
                seen.add(ch)
                nxt = deepcopy(env)
                nxt.move(int(entry.moves[e]))
                if tree["term"][ch]:                                   # a finished game: a node here, no entry there
                    value = sp._terminal_value(nxt)
                    assert value is not None and int(node[ch]) == (0 if value == sp._DRAW else value), (g, ch)
                    continue
                todo.append((ch, nxt))
        live = int(tree["n"]) - int(tree["term"][:tree["n"]].sum())
        assert len(seen) - sum(bool(tree["term"][k]) for k in seen) == live == len(player._table), g


def test_every_proof_is_sound_by_the_oracle(mirror):
    """Independent of the mirror: for every node with status +2 the oracle finds a legal move that ends the game with the
    mover as the winner, for every node with status -3 it confirms, exhaustively, that every legal move (the pass where
    there is none) allows such a reply; +1 / -1 are finished games with that winner."""
    plus2 = minus3 = 0
    for g, c in enumerate(mirror["cases"]):
        envs = _node_envs(c["tree"], c["env"])
        assert len(envs) == c["tree"]["n"]
        for k, env in envs.items():
            s = int(c["node"][k])
            over, winner = env._g.game_is_over()
            if abs(s) == 1:
                assert over and winner == (S.mover(env) if s > 0 else 3 - S.mover(env)), (g, k)
            else:
                assert not (over and winner in (1, 2)), (g, k)          # a decided game is never left unknown or deeper
            if s == 2:
                assert S.finishing_moves(env), (g, k)
                plus2 += 1
            if s == -3:
                assert S.every_move_allows_a_finishing_reply(env), (g, k)
                minus3 += 1
            assert s == 0 or env.state.turn + abs(s) - 1 <= CAP, (g, k)
    print(f"nodes at +2: {plus2}, at -3: {minus3}")
    assert plus2 >= 8 and minus3 >= 1


# ------------------------------------------------------------------------------------------ 7. off is off
@pytest.fixture(scope="module")
def near_the_end(games):
    """64 roots one to three plies before the end of 64 decisive games."""
    return _roots([games[k][0][:-(1 + k % 3)] for k in range(64)])


def _whole(ts, out, G):
    trees = [ts.export_tree(g) for g in range(G)]
    return {"out": _outputs(ts, out) + [ts.leaf_histogram().clone()], "trees": trees,
            "status": [ts.node_status(g) for g in range(G)]}


def _same_game(a, b, g, what, statuses=True):
    rows = torch.tensor([g], device="cuda")
    _same_rows(a["out"], b["out"], rows, (what, g))
    _same_tree(a["trees"][g], b["trees"][g], (what, g))
    if statuses:
        ne = a["trees"][g]["nedge"]
        assert np.array_equal(a["status"][g][0], b["status"][g][0]), (what, g)
        for k in range(a["trees"][g]["n"]):
            assert np.array_equal(a["status"][g][1][k, :ne[k]], b["status"][g][1][k, :ne[k]]), (what, g, k)


@pytest.mark.parametrize("slots", [1, 4])
def test_off_is_off_and_where_splits_the_batch(near_the_end, slots):
    G, sims = 64, 32
    rb, rh = near_the_end
    kw = {"evaluator": stub_evaluator, "noise_eps": 0.25, "slots": slots}

    def run(setup):
        ts = _search(G, sims, solver=False, **kw)
        setup(ts)
        got = _whole(ts, ts.search(rb, rh), G)
        got["stats"] = ts.solver_stats().cpu().numpy()
        ts.close()
        return got

    never = run(lambda ts: None)
    off = run(lambda ts: (ts.set_solver(True), ts.set_solver(False)))
    nowhere = run(lambda ts: ts.set_solver(True, torch.zeros(G, dtype=torch.int8)))
    for g in range(G):
        _same_game(off, never, g, "on = 0", statuses=False)
        _same_game(nowhere, never, g, "where = 0", statuses=False)
    assert not off["stats"].any() and not nowhere["stats"].any() and not never["stats"].any()
    everywhere = run(lambda ts: ts.set_solver(True))
    even = [1 - g % 2 for g in range(G)]
    mixed = run(lambda ts: ts.set_solver(True, _i8(even)))
    for g in range(G):
        # (the handle with where = 0 holds the status arrays too: a finished game's +-1 is written for every game)
        _same_game(mixed, everywhere if even[g] else nowhere, g, "mixed")
        assert np.array_equal(mixed["stats"][g], everywhere["stats"][g] if even[g] else nowhere["stats"][g]), g
    # the option did something where it was on: proofs were found and answers came from them
    changed = sum(int(everywhere["out"][0][g]) != int(never["out"][0][g]) for g in range(G))
    print("stats over the batch", everywhere["stats"].sum(0).tolist(), "answers changed", changed)
    assert everywhere["stats"][:, 1].sum() >= 1 and everywhere["stats"][:, 3].sum() >= 1


# ------------------------------------------------------------------------------------------ 8. composition
def test_budgets_and_own_clocks_equal_homogeneous_searches(games):
    """The ten win-in-one roots with budgets 1, 2, 9, 17, 40 of 40 simulations (no root noise, the host stub: the two games
    with the full budget prove their roots, as on the CPU): every game equals the search of its budget, statuses included,
    in lock step and on its own clock."""
    G, sims, cycle = len(WIN_IN_ONE), SIMS_WIN, (1, 2, 9, 17, SIMS_WIN)
    rb, rh = _roots([games[k][0][:-1] for k in WIN_IN_ONE])
    budget = [cycle[g % len(cycle)] for g in range(G)]
    budgets = torch.tensor(budget, dtype=torch.int32, device="cuda")
    kw = {"max_nodes": sims + 3}

    def run(s, b=None):
        ts = _search(G, s, **kw)
        return ts, _whole(ts, ts.search(rb, rh, budgets=b), G)

    mixed, got = run(sims, budgets)
    rolling = _search(G, sims, rolling=True, **kw)
    rolling.set_budgets(budgets)
    rolling.restart(torch.ones(G, dtype=torch.int8), rb, rh)
    done = rolling.run_rounds(mcts.rolling_quantum(sims, 1))
    assert done.tolist() == [1] * G
    rolled = _whole(rolling, rolling.policy_where(torch.ones(G, dtype=torch.int8)), G)
    proofs = 0
    for b in cycle:
        ref, want = run(b)
        for g in (g for g in range(G) if budget[g] == b):
            _same_game(got, want, g, b)
            _same_rows(rolled["out"][:6], want["out"][:6], torch.tensor([g], device="cuda"), ("rolling", b))
            _same_tree(rolled["trees"][g], want["trees"][g], ("rolling", b, g))
            assert np.array_equal(rolled["status"][g][0], want["status"][g][0]), ("rolling", b, g)
            proofs += int((want["status"][g][0] > 1).sum())
        ref.close()
    assert proofs >= 2
    mixed.close(); rolling.close()


def _breadth_first(tree, start):
    order, index = [start], {start}
    for node in order:
        for e in range(int(tree["nedge"][node])):
            c = int(tree["child"][node, e])
            if c >= 0 and c not in index:
                index.add(c)
                order.append(c)
    return order


def test_kept_trees_keep_their_statuses_and_a_proven_root_stays_proven(games):
    """keep_tree: the statuses move with the kept nodes and edges under hive_search_advance_roots' renumbering.  Game 0 is the
    recorded forced loss: its root is proven -5 at ply t, the root of the kept tree is +4 one ply on and -3 at ply t + 2,
    before a single simulation of the new search; every answer on the way comes from the proof."""
    from hive_alphazero_amd import batch
    prefixes = [_lost_game()] + [games[k][0][:-3] for k in (41, 46, 66, 78)]
    G, sims = len(prefixes), SIMS_MIRROR
    rb, rh = _roots(prefixes)
    B = batch.BoardBatch(G)
    B.import_state(rb, rh)
    ts = _search(G, sims, keep_tree=True)
    want_root = [-5, 4, -3]
    carried = 0
    played = ts.search(rb, rh)[0].clone()
    for ply in range(3):
        assert int(ts.root_status()[0]) == want_root[ply]
        before = [(ts.export_tree(g), ts.node_status(g)) for g in range(G)]
        B.step(played)
        assert B.illegal_count() == 0
        rb, rh = B.export_state()
        if ply == 2:
            break
        ts.advance_roots(rb, rh, played=played)
        kept = ts.carry_stats()[0].cpu().numpy()
        assert kept[0] > 0 and int(ts.root_status()[0]) == want_root[ply + 1]
        for g in range(G):
            old, (old_node, old_edge) = before[g]
            if kept[g] == 0:
                continue
            e = old["act"][0, :int(old["nedge"][0])].tolist().index(int(played[g]))
            order = _breadth_first(old, int(old["child"][0, e]))
            new, (node, edge) = ts.export_tree(g), ts.node_status(g)
            assert len(order) == kept[g] == new["n"]
            assert np.array_equal(node, old_node[order]), (ply, g)
            for i, k in enumerate(order):
                ne = int(old["nedge"][k])
                assert np.array_equal(edge[i, :ne], old_edge[k, :ne]), (ply, g, i)
            carried += 1
        played = ts.run_simulations()[0].clone()             # the search from the kept trees
    assert carried >= 4 and int(ts.solver_stats()[0, 3]) == 3
    ts.close(); B.close()


class _FlagStub:
    """The stub evaluator behind the row flags of hive_search_leaf_need; keeps the flags of the last batch."""
    accepts_need = True
    need = None

    def __call__(self, planes, need=None):
        self.need = need.clone()
        return _host_stub_evaluator(planes)


def test_descents_that_end_at_a_proven_node_ask_for_no_row(games):
    """The ten win-in-one roots (proven after 40 simulations) and two opening positions (never proven): in one more round
    every proven game's descent ends at its root, asks for no network row and counts as a known finished game."""
    G = len(WIN_IN_ONE) + 2
    rb, rh = _roots([games[k][0][:-1] for k in WIN_IN_ONE] + [[], games[0][0][:1]])
    ev = _FlagStub()
    ts = _search(G, SIMS_WIN, evaluator=ev)
    assert ts.skip_unread_rows
    ts.search(rb, rh)
    proven = ts.root_status().cpu().numpy() != 0
    assert proven.tolist() == [True] * (G - 2) + [False] * 2
    hist, stats = ts.leaf_histogram().cpu().numpy(), ts.solver_stats().cpu().numpy()
    ts._stream()
    ts._round(1)
    need = ev.need.cpu().numpy()
    assert not need[proven].any() and need[~proven].all()
    hist2, stats2 = ts.leaf_histogram().cpu().numpy(), ts.solver_stats().cpu().numpy()
    assert ((hist2 - hist)[proven, 3] == 1).all() and ((stats2 - stats)[proven, 0] == 1).all()
    assert ((hist2 - hist).sum(1) == 1).all() and ((stats2 - stats)[~proven] == 0).all()
    ts.close()


def test_arena_sides_with_and_without_the_option(games):
    """A searches with proven results, B without, on the ten win-in-one roots (40 simulations, no root noise; A is the host
    stub, so the roots A owns are proven as on the CPU): the games A owns come out as the solver TreeSearch with A's network
    gives them, the games B owns as the plain one with B's network, bit for bit, trees and statuses included."""
    G, sims = len(WIN_IN_ONE), SIMS_WIN
    rb, rh = _roots([games[k][0][:-1] for k in WIN_IN_ONE])
    white_to_move = (rb[:, 33] % 2 == 1).cpu().tolist()
    a_white = _i8([int(w) if g % 2 == 0 else 1 - int(w) for g, w in enumerate(white_to_move)])      # A owns the even games
    kw = {"noise_eps": 0.0, "max_nodes": sims + 3}
    arena = mcts.ArenaSearch(G, sims, _host_stub_evaluator, other_evaluator, a_white, seed=9, plane_dtype=torch.float32,
                             solver_a=True, **kw)
    arena.set_game_ids(_ids(G))
    side_a = _search(G, sims, **kw)
    side_b = _search(G, sims, solver=False, evaluator=other_evaluator, **kw)
    assert arena.solver and arena._solver_where is not None
    own_a = (a_white != 0) == (rb[:, 33] % 2 == 1)
    assert own_a.tolist() == [g % 2 == 0 for g in range(G)]
    got = _whole(arena, arena.search(rb, rh), G)
    want_a = _whole(side_a, side_a.search(rb, rh), G)
    want_b = _whole(side_b, side_b.search(rb, rh), G)
    assert torch.equal(arena._solver_where != 0, own_a)
    for g in range(G):
        _same_game(got, want_a if own_a[g] else want_b, g, "arena", statuses=bool(own_a[g]))
    stats = arena.solver_stats()
    assert (stats[own_a][:, 3] == 1).all() and not stats[~own_a].any()
    assert (arena.root_status()[own_a] == 2).all() and (arena.root_status()[~own_a] == 0).all()
    with pytest.raises(ValueError):
        mcts.ArenaSearch(G, sims, stub_evaluator, other_evaluator, a_white, gumbel_a=True, solver_b=True)
    for ts in (arena, side_a, side_b):
        ts.close()


def test_rolling_selfplay_records_equal_lock_step_records():
    """Whole short games with the option on, rolling against lock step: the packed records are equal key by key."""
    from test_gpu_rolling import _by_game, _play_out, _same_packed
    G, sims = 8, 6
    out = []
    for rolling in (None, True):
        sp = mcts.SelfPlay(G, sims, stub_evaluator, seed=21, plane_dtype=torch.float32, game_ids=range(G), packed_records=True,
                           rolling=rolling, search_options={"solver": True})
        assert sp.search.solver
        _play_out(sp)
        assert sp.env.illegal_count() == 0 and sp.finished == G and sp.dropped_games == 0
        out.append((_by_game(sp.drain_finished_packed()), sp.search.solver_stats().sum(0).tolist()))
        sp.close()
    assert sorted(out[0][0]) == sorted(out[1][0]) == list(range(G))
    for gid in range(G):
        _same_packed(out[0][0][gid], out[1][0][gid])
    assert out[0][1] == out[1][1]


# ------------------------------------------------------------------------------------------ refusals
def test_what_the_handle_refuses():
    from hive_alphazero_amd import _lib
    with pytest.raises(ValueError):
        mcts.TreeSearch(2, 4, stub_evaluator, mode=mcts.UCT, solver=True)
    with pytest.raises(ValueError):
        mcts.TreeSearch(2, 4, stub_evaluator, gumbel=True, solver=True)
    ts = mcts.TreeSearch(2, 4, stub_evaluator, plane_dtype=torch.float32, solver=True)
    with pytest.raises(ValueError):
        ts.set_gumbel(True)
    prm = mcts._GumbelParams(16, 50.0, 1.0, 4)
    import ctypes
    assert ts.L.hive_search_set_gumbel(ts._h, ctypes.byref(prm), None) == -1          # HIVE_E_ARG
    uct = mcts._Params(0.7, 0.0, 0.3, 250, mcts.UCT, 0.0)
    assert ts.L.hive_search_set_params(ts._h, ctypes.byref(uct)) == -1
    ts.set_solver(False)
    ts.set_gumbel(True)
    assert ts.L.hive_search_set_solver(ts._h, 1, None) == -1
    assert "Gumbel" in ts.L.hive_last_error().decode()
    ts.close()
    assert _lib.HiveError is not None
