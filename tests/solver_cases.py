"""Positions near the end of seeded `crowd` games (env_corpus) for the solver tests, the sequential player on them, and
the rules restated with the CPU oracle.  TEST INFRASTRUCTURE, CPU-only: imported by tests, never by the product package."""
from copy import deepcopy

import numpy as np

import env_corpus as C
from mcts_stub import StubPipe
from oracle import oracle_py as O
from oracle_env import OracleGamePlay

CAP = 55


def decisive_games(n, seed):
    """n `crowd` games that end with a winner, as move lists (env_corpus.play_game with the moves kept: the same draws from
    the same generator, so game k here is the k-th decisive game of env_corpus.finished_with_previous's stream)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        g, moves = O.OracleGame(), []
        while True:
            p = C.snapshot(g)
            if p.over or p.turn >= C.MAX_TURN:
                break
            a = C.choose("crowd", p, rng, None)
            moves.append(a)
            g.move(a)
        if p.over and p.winner in (1, 2):
            out.append((moves, p.winner))
    return out


def env_after(moves):
    g = OracleGamePlay()
    for a in moves:
        g.move(int(a))
    return g


def mover(env):
    """1 white, 2 black: the side to move, in the oracle's winner code."""
    return 1 if env.state.turn % 2 == 1 else 2


def finishing_moves(env):
    """The legal moves of env's position that end the game with its mover as the winner."""
    me, out = mover(env), []
    for a in env.actions():
        nxt = deepcopy(env)
        nxt.move(a)
        over, w = nxt._g.game_is_over()
        if over and w == me:
            out.append(int(a))
    return out


def every_move_allows_a_finishing_reply(env):
    """Exhaustively: the position is not finished, and after every legal move (the pass when there is none) the game goes
    on and the opponent has a move that ends it with the opponent as the winner."""
    over, _ = env._g.game_is_over()
    if over:
        return False
    for a in (env.actions() or [-1]):
        nxt = deepcopy(env)
        nxt.move(a)
        if nxt._g.game_is_over()[0] or not finishing_moves(nxt):
            return False
    return True


def player(sims, solver):
    """The sequential player without root noise on the stub evaluator."""
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    p = sp.HivePlayer(pipes=[StubPipe()])
    p.simulation_num_per_move = sims
    p.solver = solver
    return p


def run_player(env, sims, solver, seed=0):
    """-> (player, move, policy float64[1584], visits) with noise_eps = 0 (deterministic) and numpy's stream restored."""
    import hive_alphazero_amd.solo_play as sp
    p = player(sims, solver)
    state, old = np.random.get_state(), sp.noise_eps
    sp.noise_eps = 0.0
    try:
        np.random.seed(seed)
        move, (policy, visits) = p.action(env)
    finally:
        sp.noise_eps = old
        np.random.set_state(state)
    return p, int(move), np.asarray(policy, dtype=np.float64), int(visits)
