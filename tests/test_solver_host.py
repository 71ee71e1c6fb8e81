"""Proven wins and losses below the root, host side (no GPU): the four numpy statements of search_rules on hand-made rows, the
sequential player (solo_play.HivePlayer.solver) on win-in-one roots of the CPU oracle env, the refusals, and the ABI's
declarations."""
import os

import numpy as np
import pytest

import solver_cases as S
from hive_alphazero_amd import search_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 1. the rule on hand-made rows
def test_edge_status_is_the_child_seen_from_the_mover():
    assert R.solver_edge_status(0) == 0                      # a draw child, a capped child, an unknown child: nothing
    assert R.solver_edge_status(+1) == -2                    # the child's side to move has won: the move lost
    assert R.solver_edge_status(-1) == +2                    # the finishing move
    assert R.solver_edge_status(+2) == -3 and R.solver_edge_status(-3) == +4 and R.solver_edge_status(-126) == 127
    assert R.solver_edge_status(np.array([0, 1, -1, 4])).tolist() == [0, -2, 2, -5]


def test_node_status_from_all_edges():
    assert R.solver_node_status([-3, -5, +4, 0]) == 4        # any win beats losses and unknowns
    assert R.solver_node_status([-3, +6, +2, +4]) == 2       # the fastest win
    assert R.solver_node_status([-3, -7, -5]) == -7          # every move loses: the longest resistance
    assert R.solver_node_status([-3, 0, -5]) == 0            # an unexpanded edge (status 0) blocks the loss proof
    assert R.solver_node_status([-3]) == -3                  # the pass edge is an edge like any other
    assert R.solver_node_status([+2]) == 2
    assert R.solver_node_status([0]) == 0 and R.solver_node_status([]) == 0
    # a draw child proves nothing: its edge stays 0 and keeps the node open
    assert R.solver_node_status([R.solver_edge_status(0), R.solver_edge_status(+1)]) == 0


def test_holds_up_to_the_length_cap():
    cap = 55
    for x in (2, -2):
        assert R.solver_holds(x, 54, cap)                    # T + |x| - 1 == cap
        assert not R.solver_holds(x, 55, cap)                # one above
    assert R.solver_holds(-5, 51, cap) and not R.solver_holds(-5, 52, cap)
    assert R.solver_holds(1, 55, cap) and not R.solver_holds(0, 1, cap)
    assert R.solver_holds(np.array([0, 2, -4, 3]), 53, cap).tolist() == [False, True, False, True]


def test_answer_and_its_ties():
    cap = 55
    # a proven win: the smallest positive status; ties to more visits, then to the lower edge
    assert R.solver_answer([0, 4, 2, -3], [9, 5, 1, 0], 10, cap)[0] == 2
    assert R.solver_answer([2, 0, 2, 2], [1, 9, 3, 3], 10, cap)[0] == 2
    assert R.solver_answer([2, 2], [3, 3], 10, cap)[0] == 0
    # a proven loss: the largest |e|, same ties
    assert R.solver_answer([-3, -5, -5], [9, 1, 2], 10, cap)[0] == 2
    assert R.solver_answer([-3, -3], [2, 2], 10, cap)[0] == 0
    assert R.solver_answer([-3], [0], 10, cap)[0] == 0       # the pass edge
    # no proof: the losing moves leave the choice
    edge, allowed = R.solver_answer([-3, 0, -5, 0], [5, 1, 1, 1], 10, cap)
    assert edge == -1 and allowed.tolist() == [False, True, False, True]
    # at the cap a status that does not hold is 0: the win in 3 plies is out of reach at turn 53, the one in 1 is not
    assert R.solver_answer([4, 2], [1, 1], 53, cap)[0] == 1
    edge, allowed = R.solver_answer([4, 0], [1, 1], 53, cap)
    assert edge == -1 and allowed.all()
    edge, allowed = R.solver_answer([-5, -3], [1, 1], 52, cap)          # -5 does not hold at 52: the root is not lost
    assert edge == -1 and allowed.tolist() == [True, False]
    assert R.solver_answer([-5, -3], [1, 1], 51, cap)[0] == 0


# ------------------------------------------------------------------------------------------ 2. the sequential player
SIMS = 40
WIN_IN_ONE = [15, 19, 45, 53, 137, 159, 168, 189, 228, 332]      # of decisive_games(333, 11), cut one ply before the end


@pytest.fixture(scope="module")
def games():
    return S.decisive_games(max(WIN_IN_ONE) + 1, 11)


def test_player_plays_the_finishing_move_it_has_seen(games):
    """Ten win-in-one roots at which the plain player, after 40 simulations, answers another move although the finishing
    edge was expanded.  With `solver` the root is +2 from the simulation that expands that edge, every later descent ends
    at the root, and the answer is the finishing move."""
    for k in WIN_IN_ONE:
        moves, winner = games[k]
        env = S.env_after(moves[:-1])
        assert winner == S.mover(env)
        finishing = S.finishing_moves(env)
        assert moves[-1] in finishing
        plain, plain_move, plain_policy, plain_visits = S.run_player(env, SIMS, False)
        assert plain_move not in finishing and plain_visits == SIMS - 1
        assert plain.solver_stats == [0, 0, 0, 0] and plain._table[env.state_key].status == 0
        solved, move, policy, visits = S.run_player(env, SIMS, True)
        root = solved._table[env.state_key]
        assert move in finishing and root.status == 2
        edge = root.moves.index(move)
        assert root.es[edge] == 2 and root.n[edge] == 1 and root.w[edge] == 1.0
        stops, wins, losses, answers = solved.solver_stats
        assert (wins, losses, answers) == (1, 0, 1)
        # the simulations after the proof ended at the root: they are the visits the policy row is short of
        assert visits == SIMS - 1 - stops and abs(policy.sum() - 1.0) < 1e-12
        # up to the proving simulation the two searches are one: the plain tree after `visits` + 1 simulations
        short, _, short_policy, short_visits = S.run_player(env, visits + 1, False)
        assert short_visits == visits and np.array_equal(short_policy, policy)
        assert short._table[env.state_key].n.tolist() == root.n.tolist()


def test_player_without_the_option_is_unchanged(games):
    import hive_alphazero_amd.solo_play as sp
    moves, _ = games[WIN_IN_ONE[0]]
    env = S.env_after(moves[:-1])
    assert sp.HivePlayer.solver is False
    a, move_a, policy_a, _ = S.run_player(env, SIMS, False)
    b = S.player(SIMS, None)
    del b.solver                                             # the class default
    old = sp.noise_eps
    sp.noise_eps = 0.0
    state = np.random.get_state()
    try:
        np.random.seed(0)
        move_b, (policy_b, _) = b.action(env)
        after_b = np.random.get_state()[1].copy()
        np.random.seed(0)
        S.player(SIMS, False).action(env)
        after_a = np.random.get_state()[1]
    finally:
        sp.noise_eps = old
        np.random.set_state(state)
    assert move_a == move_b and np.array_equal(policy_a, np.asarray(policy_b)) and np.array_equal(after_a, after_b)
    for key, e in a._table.items():
        f = b._table[key]
        assert e.status == f.status == 0
        if e.moves is not None:
            assert e.n.tolist() == f.n.tolist() and e.w.tolist() == f.w.tolist() and not e.es.any()


def test_the_recorded_forced_loss_is_one():
    """tests/golden/solver_lost_game.json: after 23 plies the side to move cannot move and every continuation loses."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "solver_lost_game.json")) as f:
        rec = json.load(f)
    env = S.env_after(rec["moves"][:rec["lost_after_plies"]])
    assert env.actions() == [] and S.every_move_allows_a_finishing_reply(env)
    solved, move, _, _ = S.run_player(env, 48, True)
    statuses = sorted(e.status for e in solved._table.values() if e.status)
    assert solved._table[env.state_key].status == -5 and move == -1 and statuses == [-5, -3, 2, 4]


# ------------------------------------------------------------------------------------------ 3. refusals and declarations
def test_solver_options_refusals():
    assert R.solver_options(None) is False and R.solver_options(False) is False and R.solver_options(True) is True
    with pytest.raises(ValueError):
        R.solver_options(True, mode=R.UCT)
    with pytest.raises(ValueError):
        R.solver_options(True, gumbel={"m": 16})
    with pytest.raises(ValueError):
        R.solver_options(True, gumbel=True)
    with pytest.raises(ValueError):
        R.solver_options({"depth": 3})
    assert R.solver_options(False, mode=R.UCT, gumbel=True) is False
    import hive_alphazero_amd.solo_play as sp
    p = S.player(4, True)
    p.gumbel = {"m": 4}
    with pytest.raises(ValueError):
        p.action(S.env_after([]))
    assert sp.HivePlayer.solver is False


def test_header_declares_the_calls_and_states_the_rule_once():
    from hive_alphazero_amd._lib import ABI_SYMBOLS
    with open(os.path.join(ROOT, "include", "hive_search.h")) as f:
        text = f.read()
    for name in ("hive_search_set_solver", "hive_search_node_status", "hive_search_root_status", "hive_search_solver_stats"):
        assert f"int {name}(" in text and name in ABI_SYMBOLS
    assert text.count("e_status[P][k] = -sign(c) * (|c| + 1)") == 1
