"""Gumbel selection below the root on the GPU (hive_search_set_gumbel_interior, hive_search_node_values): the search against
the sequential statement over the whole tree, the `where` mask bit for bit, the first choice at a fresh node, budgets and
per-game clocks, node values under tree reuse, the arena's per-side option and a short self-play."""
from copy import deepcopy

import numpy as np
import pytest
import torch

from hive_alphazero_amd import mcts
from mcts_stub import StubPipe
from test_gpu_gumbel import (_host_stub_evaluator, _ids, _outputs, _roots, _same_rows, _same_tree, other_evaluator,
                             stub_evaluator)

pytestmark = pytest.mark.gpu

SIMS = 33
M = SIMS + 3


def _search(G, sims, gumbel=True, interior=False, evaluator=stub_evaluator, seed=9, **kw):
    ts = mcts.TreeSearch(G, sims, evaluator, plane_dtype=torch.float32, seed=seed, gumbel=gumbel, gumbel_interior=interior, **kw)
    ts.set_game_ids(_ids(G))
    return ts


def _i8(x):
    return torch.tensor(x, dtype=torch.int8, device="cuda")


# ------------------------------------------------------------------------------------------ 1. the sequential statement
@pytest.mark.parametrize("quiet", [False, True])
@pytest.mark.parametrize("prefix_seed,plies", [(21, 0), (22, 3), (23, 8), (24, 14)])
def test_whole_tree_matches_the_sequential_statement(prefix_seed, plies, quiet):
    """33 simulations, m = 16, one game, the host stub evaluator on both sides; noisy with the mirror fed gumbel_draw, and
    quiet.  The GPU tree and the mirror's table are walked together from the root by action id: every edge of every node
    reached holds the same N, every node the value the mirror's entry was predicted with.  fp32 against float64: meaningful
    away from near-ties, so the mirror's smallest strictly positive top-two gap -- root and interior selections -- is asserted
    to be at least 1e-4.  On the CPU (oracle env) the eight cases give 3.7e-4 .. 2.2e-3, the interior selections alone
    3.9e-4 .. 2.2e-3; the listed seeds all pass, none was replaced."""
    import hive_alphazero_amd.solo_play as sp
    from hive_alphazero_amd import batch
    from hive_alphazero_amd.env_hive import GamePlay
    rng = np.random.default_rng(prefix_seed)
    g = GamePlay(1050, 900)
    for _ in range(plies):
        acts = g.actions()
        g.move(int(acts[rng.integers(len(acts))]))
    seed = 3
    sp.SEARCH_THREADS = 1
    player = sp.HivePlayer(pipes=[StubPipe()])
    player.simulation_num_per_move = SIMS
    player.gumbel = {"m": 16, "interior": True,
                     "g": None if quiet else (lambda turn, ne: mcts.gumbel_draw(seed, 0, turn, ne))}
    move, (ref_policy, ref_visits) = player.action(g)
    print(f"min gap {player.gumbel_min_gap:.3g} interior {player.gumbel_interior_min_gap:.3g} "
          f"fallbacks {player.gumbel_fallbacks} entries {len(player._table)}")
    assert player.gumbel_min_gap >= 1e-4
    assert player.gumbel_interior_min_gap < float("inf")           # the rule was used
    B = batch.BoardBatch(1)
    B.import_state(g._rec.reshape(1, 64), g._hist.reshape(1, 384))
    rb, rh = B.export_state()
    ts = mcts.TreeSearch(1, SIMS, _host_stub_evaluator, plane_dtype=torch.float32, seed=seed, gumbel={"m": 16},
                         gumbel_interior=True, max_nodes=M)
    kw = {"budgets": torch.tensor([SIMS], dtype=torch.int32, device="cuda"),
          "quiet": torch.ones((1,), dtype=torch.int8, device="cuda")} if quiet else {}
    action, policy, sum_n = ts.search(rb, rh, **kw)
    assert int(action[0]) == move and int(sum_n[0]) == int(ref_visits) == SIMS - 1
    assert np.abs(policy[0].cpu().numpy().astype(np.float64) - np.asarray(ref_policy)).max() < 1e-5
    assert int(ts.gumbel_fallbacks()[0]) == player.gumbel_fallbacks
    tree, values = ts.export_tree(0), ts.node_values(0)
    assert values.shape == (tree["n"],) and values.dtype == np.float32
    # walk both from the root: GPU node k <-> the mirror's entry of the position reached
    todo, seen, opened, deep = [(0, deepcopy(g), 0)], {0}, 0, 0
    while todo:
        k, env, depth = todo.pop()
        assert not tree["term"][k]
        entry = player._table[env.state_key]
        assert abs(float(values[k]) - entry.v) <= 1e-6, (k, depth)
        ne = int(tree["nedge"][k])
        if entry.moves is None:                                    # evaluated, never selected: no visit below it
            assert not tree["n_visits"][k, :ne].any() and int(tree["sum_n"][k]) == 0, k
            continue
        assert tree["act"][k, :ne].tolist() == list(entry.moves), k
        assert tree["n_visits"][k, :ne].tolist() == entry.n.tolist(), (k, depth)
        opened += 1
        deep = max(deep, depth)
        for e in range(ne):
            c = int(tree["child"][k, e])
            assert c >= -1
            if c < 0 or c in seen:
                continue
            nxt = deepcopy(env)
            nxt.move(int(entry.moves[e]))
            if tree["term"][c]:                                    # a finished game has a node here and no entry there
                assert sp._terminal_value(nxt) is not None and nxt.state_key not in player._table
                assert float(values[c]) == float(tree["tv"][c])
                continue
            seen.add(c)
            todo.append((c, nxt, depth + 1))
    # every expanded node was reached and is an entry of the mirror
    live = int(tree["n"]) - int(tree["term"][:tree["n"]].sum())
    assert len(seen) == live == len(player._table) and opened >= 2 and deep >= 1
    ts.close(); B.close()


# ------------------------------------------------------------------------------------------ 2. / 3. where
@pytest.fixture(scope="module")
def split():
    """64 games, 33 simulations: root-only Gumbel, and the same with the interior rule on the even games."""
    G = 64
    rb, rh = _roots(G, seed=7, games=8, skip=16)
    even = _i8([1 - g % 2 for g in range(G)])
    root_only = _search(G, SIMS, max_nodes=M)
    want = _outputs(root_only, root_only.search(rb, rh))
    half = _search(G, SIMS, max_nodes=M)
    half.set_gumbel_interior(True, even)
    got = _outputs(half, half.search(rb, rh))
    out = {"G": G, "rb": rb, "rh": rh, "even": even, "want": want, "got": got,
           "want_trees": [root_only.export_tree(g) for g in range(G)], "got_trees": [half.export_tree(g) for g in range(G)]}
    root_only.close(); half.close()
    return out


def test_option_changes_the_descent_only_where_asked(split):
    G, even = split["G"], split["even"]
    odd_rows = torch.nonzero(even == 0).view(-1)
    _same_rows(split["got"], split["want"], odd_rows, "odd games")
    for g in odd_rows.tolist():
        _same_tree(split["got_trees"][g], split["want_trees"][g], g)
    # the even games: the rule is another descent -- some tree differs in a node below the root's children
    below = 0
    for g in range(0, G, 2):
        a, b = split["got_trees"][g], split["want_trees"][g]
        kids_a = {int(c) for c in a["child"][0, :int(a["nedge"][0])] if c >= 0}
        kids_b = {int(c) for c in b["child"][0, :int(b["nedge"][0])] if c >= 0}
        # the boards of the nodes at depth >= 2, as a set: another choice at a depth-1 node expands another position
        deep_a = {a["board"][k].tobytes() for k in range(1, a["n"]) if k not in kids_a}
        deep_b = {b["board"][k].tobytes() for k in range(1, b["n"]) if k not in kids_b}
        below += int(deep_a != deep_b)
        assert int(split["got"][2][g]) == int(split["want"][2][g])          # the root's budget is spent either way
    print(f"even games whose tree differs below depth 1: {below} of {G // 2}")
    assert below >= 1


def test_games_without_the_gumbel_root_are_plain_puct_searches(split):
    """The root's `where` at 0 on every fourth game, the interior option on for all: those games are the plain PUCT search,
    and a handle whose Gumbel root is off does not notice the option at all."""
    G, rb, rh = split["G"], split["rb"], split["rh"]
    where = _i8([int(g % 4 != 3) for g in range(G)])
    off_rows = torch.nonzero(where == 0).view(-1)
    plain = _search(G, SIMS, gumbel=None, max_nodes=M)
    want = _outputs(plain, plain.search(rb, rh))
    option_only = _search(G, SIMS, gumbel=None, max_nodes=M)
    option_only.set_gumbel_interior(True)                          # accepted before (and without) hive_search_set_gumbel
    _same_rows(_outputs(option_only, option_only.search(rb, rh)), want, torch.arange(G, device="cuda"), "option alone")
    mixed = _search(G, SIMS, interior=True, max_nodes=M)
    mixed.set_gumbel_where(where)
    assert mixed.gumbel_interior
    got = _outputs(mixed, mixed.search(rb, rh))
    _same_rows(got, want, off_rows, "no Gumbel root")
    for g in off_rows.tolist():
        _same_tree(mixed.export_tree(g), plain.export_tree(g), g)
        _same_tree(option_only.export_tree(g), plain.export_tree(g), ("option alone", g))
    # Gumbel off and on again: the interior setting is as it was -- the even games of `split` come out again
    mixed.set_gumbel(None)
    mixed.set_gumbel(True)
    assert mixed.gumbel_interior
    mixed.set_gumbel_interior(True, split["even"])
    again = _outputs(mixed, mixed.search(rb, rh))
    _same_rows(again, split["got"], torch.arange(G, device="cuda"), "off and on")
    mixed.set_gumbel_interior(False)
    _same_rows(_outputs(mixed, mixed.search(rb, rh)), split["want"], torch.arange(G, device="cuda"), "option off")
    plain.close(); option_only.close(); mixed.close()


def test_fresh_interior_node_follows_its_priors(split):
    """A depth-1 node with exactly one visited child: while nothing below it was visited the improved policy is the priors,
    so its first choice -- and, with one visited child, every choice so far -- is their argmax, lowest edge on ties."""
    checked = 0
    for g in range(0, split["G"], 2):
        t = split["got_trees"][g]
        for c in {int(c) for c in t["child"][0, :int(t["nedge"][0])] if c >= 0}:
            ne = int(t["nedge"][c])
            visited = np.flatnonzero(t["n_visits"][c, :ne] > 0)
            if t["term"][c] or len(visited) != 1:
                continue
            assert int(visited[0]) == int(np.argmax(t["p"][c, :ne])), (g, c)
            checked += 1
    assert checked >= 32


# ------------------------------------------------------------------------------------------ 4. budgets and rolling
def test_mixed_budgets_and_own_clocks_equal_homogeneous_searches():
    G, cycle = 10, (1, 2, 9, 17, 33)
    rb, rh = _roots(G, seed=17, games=4, skip=12)
    budget = [cycle[g % len(cycle)] for g in range(G)]
    budgets = torch.tensor(budget, dtype=torch.int32, device="cuda")

    def run(s, b=None):
        ts = _search(G, s, interior=True, max_nodes=M)
        return ts, _outputs(ts, ts.search(rb, rh, budgets=b))

    mixed, got = run(SIMS, budgets)
    rolling = _search(G, SIMS, interior=True, max_nodes=M, rolling=True)
    rolling.set_budgets(budgets)
    rolling.restart(torch.ones(G, dtype=torch.int8), rb, rh)
    done = rolling.run_rounds(mcts.rolling_quantum(SIMS, 1))
    assert done.tolist() == [1] * G
    rolled = _outputs(rolling, rolling.policy_where(torch.ones(G, dtype=torch.int8)))
    _same_rows(rolled, got, torch.arange(G, device="cuda"), "rolling")
    for b in cycle:
        ref, want = run(b)
        rows = torch.tensor([g for g in range(G) if budget[g] == b], device="cuda")
        _same_rows(got, want, rows, b)
        assert (got[0][rows] >= -1).all() and (got[2][rows] == b - 1).all()
        for g in rows.tolist():
            _same_tree(mixed.export_tree(g), ref.export_tree(g), (b, g))
            _same_tree(rolling.export_tree(g), ref.export_tree(g), ("rolling", b, g))
            assert np.array_equal(mixed.node_values(g).view(np.uint32), ref.node_values(g).view(np.uint32))
        ref.close()
    mixed.close(); rolling.close()


# ------------------------------------------------------------------------------------------ 5. node values under tree reuse
def _breadth_first(tree, start):
    """Old node ids in the order hive_search_advance_roots renumbers them: breadth first from `start` in edge order."""
    order, index = [start], {start}
    for node in order:
        for e in range(int(tree["nedge"][node])):
            c = int(tree["child"][node, e])
            if c >= 0 and c not in index:
                index.add(c)
                order.append(c)
    return order


def test_kept_nodes_keep_their_values():
    from hive_alphazero_amd import batch
    G, sims = 13, 24
    rb, rh = _roots(G, seed=19, games=4, skip=12)
    B = batch.BoardBatch(G)
    B.import_state(rb, rh)
    ts = mcts.TreeSearch(G, sims, stub_evaluator, plane_dtype=torch.float32, seed=5, keep_tree=True)
    played = ts.search(rb, rh)[0].clone()
    before = [(ts.export_tree(g), ts.node_values(g)) for g in range(G)]
    for tree, values in before:
        # a node holds the value it was created with: tv for a finished game, a network value otherwise
        term = tree["term"].astype(bool)
        assert np.array_equal(values[term].view(np.uint32), tree["tv"][term].view(np.uint32))
        assert (np.abs(values[~term]) <= 0.9).all() and len(np.unique(values[~term])) > 1
    B.step(played)
    assert B.illegal_count() == 0
    rb2, rh2 = B.export_state()
    ts.advance_roots(rb2, rh2, played=played)
    kept = ts.carry_stats()[0].cpu().numpy()
    carried, nodes, orders = 0, 0, {}
    for g in range(G):
        old, old_v = before[g]
        new, new_v = ts.export_tree(g), ts.node_values(g)
        assert new["n"] == kept[g] == len(new_v)
        if kept[g] == 0:
            continue
        edge = [e for e in range(int(old["nedge"][0])) if old["act"][0, e] == int(played[g])]
        child = int(old["child"][0, edge[0]])
        order = orders[g] = _breadth_first(old, child)
        assert len(order) == kept[g]
        assert np.array_equal(new_v.view(np.uint32), old_v[order].view(np.uint32)), g
        assert new_v.view(np.uint32)[0] == old_v.view(np.uint32)[child]            # node 0's value is its old child's
        carried += 1
        nodes += len(order)
    assert carried >= G // 2 and nodes > carried
    # the next search from the kept trees writes the new nodes' values behind the kept ones
    ts.run_simulations()
    for g, order in orders.items():
        new_v = ts.node_values(g)
        assert len(new_v) > len(order), g
        assert np.array_equal(new_v[:len(order)].view(np.uint32), before[g][1][order].view(np.uint32)), g
    ts.close(); B.close()


# ------------------------------------------------------------------------------------------ 6. arena
def test_arena_full_gumbel_against_root_only_gumbel():
    """Both sides search with the Gumbel root, A also below it.  The games A owns must come out as the full-Gumbel TreeSearch
    with A's network gives them, the games B owns as the root-only one with B's network, bit for bit, trees included."""
    from hive_alphazero_amd import batch
    G, sims = 16, 17
    rb, rh = _roots(G, seed=41, games=8, skip=16)
    a_white = _i8([1, 0] * (G // 2))
    arena = mcts.ArenaSearch(G, sims, stub_evaluator, other_evaluator, a_white, seed=9, plane_dtype=torch.float32,
                             gumbel_a=True, gumbel_b=True, gumbel_interior_a=True, max_nodes=sims + 3)
    side_a = _search(G, sims, interior=True, max_nodes=sims + 3)
    side_b = _search(G, sims, evaluator=other_evaluator, max_nodes=sims + 3)
    arena.set_game_ids(_ids(G))
    assert arena._gumbel_where is None and arena._gumbel_interior_where is not None and arena.gumbel_interior
    B = batch.BoardBatch(G)
    B.import_state(rb, rh)
    owned, differ = [0, 0], 0
    for ply in range(2):
        rb, rh = B.export_state()
        own_a = (a_white != 0) == (rb[:, 33] % 2 == 1)
        got = _outputs(arena, arena.search(rb, rh))
        want_a = _outputs(side_a, side_a.search(rb, rh))
        want_b = _outputs(side_b, side_b.search(rb, rh))
        _same_rows(got, want_a, torch.nonzero(own_a).view(-1), ("A", ply))
        _same_rows(got, want_b, torch.nonzero(~own_a).view(-1), ("B", ply))
        assert torch.equal(arena._gumbel_interior_where != 0, own_a)
        for g in range(G):
            _same_tree(arena.export_tree(g), (side_a if own_a[g] else side_b).export_tree(g), (ply, g))
        owned[0] += int(own_a.sum())
        owned[1] += int((~own_a).sum())
        B.step(got[0])
    assert min(owned) >= 4 and B.illegal_count() == 0
    with pytest.raises(ValueError):
        mcts.ArenaSearch(G, sims, stub_evaluator, other_evaluator, a_white, gumbel_a=True, gumbel_interior_b=True)
    for ts in (arena, side_a, side_b):
        ts.close()
    B.close()


# ------------------------------------------------------------------------------------------ 7. self-play
def test_short_selfplay_with_the_interior_rule_plays_legal_games():
    from test_gpu_scale import _replay_game_through_the_oracle
    G = 8
    sp = mcts.SelfPlay(G, 9, stub_evaluator, seed=21, plane_dtype=torch.float32, game_ids=range(G), max_finished_kept=2 * G,
                       search_options={"gumbel": True, "gumbel_interior": True})
    assert sp.search.gumbel is not None and sp.search.gumbel_interior
    games = []
    for _ in range(60):
        sp.play_ply()
        games += sp.drain_finished()
        if sp.running() == 0:
            break
    torch.cuda.synchronize()
    assert sp.running() == 0 and len(games) == G and sp.dropped_games == 0 and sp.env.illegal_count() == 0
    assert sorted(e[2] for e in games) == list(range(G))
    plies = 0
    for value_white, rows, gid in games:
        plies += _replay_game_through_the_oracle(value_white, rows, gid)[0]
    assert plies >= 8 * G
    sp.close()
