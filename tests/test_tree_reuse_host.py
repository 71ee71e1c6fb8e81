"""HivePlayer.keep_tree (solo_play.py): the sequential statement of what hive_search_advance_roots keeps -- the entries
reachable from the new position through visited edges -- on the CPU oracle env."""
from copy import deepcopy

import numpy as np

from mcts_stub import StubPipe
from oracle_env import OracleGamePlay


def _position(prefix_seed, plies):
    rng = np.random.default_rng(prefix_seed)
    g = OracleGamePlay()
    for _ in range(plies):
        acts = g.actions()
        g.move(int(acts[rng.integers(len(acts))]))
    return g


def _player(sp, sims, keep):
    player = sp.HivePlayer(pipes=[StubPipe()])
    player.keep_tree = keep
    player.simulation_num_per_move = sims
    return player


def _closure(player, env):
    """Keys reachable from env through edges with n > 0, computed on the public tree view alone."""
    seen, todo = set(), [deepcopy(env)]
    while todo:
        at = todo.pop(0)
        over = at.game_is_over() or at.state.turn >= 55
        if over or at.state_key in seen or at.state_key not in player.tree:
            continue
        seen.add(at.state_key)
        for move, edge in player.tree[at.state_key].a.items():
            if edge.n > 0:
                nxt = deepcopy(at)
                nxt.move(move)
                todo.append(nxt)
    return seen


def _snapshot(player, keys):
    return {k: (player.tree[k].sum_n, {m: (e.n, e.w, float(e.p)) for m, e in player.tree[k].a.items()}) for k in keys}


def test_keep_tree_prunes_the_table_to_the_closure_of_the_new_position():
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    assert sp.HivePlayer.keep_tree is False
    sims = 30
    for prefix_seed, plies in ((22, 3), (23, 8), (24, 14)):
        g = _position(prefix_seed, plies)
        player = _player(sp, sims, True)
        np.random.seed(1)
        move, _ = player.action(g)
        size = len(player.tree)
        assert size > 1 and player.tree[g.state_key].sum_n == sims - 1
        through = player.tree[g.state_key].a[move].n          # simulations that went through the played edge
        assert through > 1
        g.move(move)
        want = _closure(player, g)
        stats = _snapshot(player, want)
        assert 1 < len(want) < size and g.state_key in want
        # the first of those simulations evaluated the child, every later one passed one of its edges
        assert player.tree[g.state_key].sum_n == through - 1
        player.keep_reachable(g)
        assert len(player.tree) == len(want) and all(k in player.tree for k in want)
        assert _snapshot(player, want) == stats
        move2, (policy, visits) = player.action(g)              # keeps, then searches
        assert all(k in player.tree for k in want)
        assert player.tree[g.state_key].sum_n == through - 1 + sims == int(visits)
        assert len(player.tree) > len(want) and move2 in g.actions()


def test_keep_tree_off_is_the_reference_reset():
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    sims = 30
    g = _position(23, 8)
    player = _player(sp, sims, False)
    np.random.seed(1)
    move, _ = player.action(g)
    g.move(move)
    np.random.seed(2)
    again = player.action(g)
    fresh = _player(sp, sims, False)
    np.random.seed(2)
    ref = fresh.action(g)
    assert len(player.tree) == len(fresh.tree) and again[0] == ref[0] and again[1] == ref[1]
    assert player.tree[g.state_key].sum_n == sims - 1
