"""Gumbel selection below the root, host side (no GPU): the sequential statement (solo_play.HivePlayer.gumbel with
"interior") on the CPU oracle env, the rule restated in numpy on hand-made rows, the option plumbing with its refusals, and
the ABI's declarations."""
import os

import numpy as np
import pytest

from hive_alphazero_amd import mcts
from mcts_stub import StubPipe
from oracle_env import OracleGamePlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _position(prefix_seed, plies):
    rng = np.random.default_rng(prefix_seed)
    g = OracleGamePlay()
    for _ in range(plies):
        acts = g.actions()
        g.move(int(acts[rng.integers(len(acts))]))
    return g


def _player(sims, **gumbel):
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    player = sp.HivePlayer(pipes=[StubPipe()])
    player.simulation_num_per_move = sims
    player.gumbel = gumbel
    return player


def _table(player):
    """The whole table as plain data: state key -> (moves, n, w, v)."""
    return {k: (list(e.moves or []), None if e.n is None else e.n.tolist(), None if e.w is None else e.w.tolist(), e.v)
            for k, e in player._table.items()}


# ------------------------------------------------------------------------------------------ the sequential statement
@pytest.mark.parametrize("prefix_seed,plies", [(21, 0), (22, 3), (23, 8), (24, 14)])
def test_interior_mirror_is_deterministic_and_keeps_the_root_schedule(prefix_seed, plies):
    sims, M = 33, 16
    g = _position(prefix_seed, plies)
    ne = len(g.actions())
    state = np.random.get_state()
    first = _player(sims, m=M, interior=True)
    move, (policy, visits) = first.action(g)
    again = _player(sims, m=M, interior=True)
    move2, (policy2, visits2) = again.action(g)
    assert np.array_equal(state[1], np.random.get_state()[1])      # no draw of any kind: numpy's stream is untouched
    assert move == move2 and visits == visits2 and policy == policy2
    assert _table(first) == _table(again) and len(first._table) > 2
    # the root still spends its visits by the halving schedule
    root = first.tree[g.state_key]
    slots = [0] * ne
    for t in mcts.gumbel_considered_visits(min(M, ne), sims - 1).tolist():
        slots[slots.index(t)] += 1
    assert first.gumbel_fallbacks == 0 and int(visits) == sims - 1 == root.sum_n
    assert sorted(e.n for e in root.a.values()) == sorted(slots)
    assert 0 < first.gumbel_min_gap <= first.gumbel_interior_min_gap
    # every entry remembers the value its position was predicted with
    assert all(isinstance(e.v, float) and -1.0 <= e.v <= 1.0 for e in first._table.values())
    assert first._table[g.state_key].v == first._root_v
    # and the rule is what the descent used: root-only Gumbel builds another tree from the same position
    root_only = _player(sims, m=M)
    root_only.action(g)
    assert root_only.gumbel_interior_min_gap == float("inf")
    assert _table(root_only) != _table(first)


def test_default_mirror_does_not_read_the_new_key():
    g = _position(22, 3)
    a, b = _player(17, m=16), _player(17, m=16, interior=False)
    assert a.action(g)[0] == b.action(g)[0] and _table(a) == _table(b)


# ------------------------------------------------------------------------------------------ the rule, restated
C_VISIT, C_SCALE, C_PUCT = 50.0, 1.0, 0.7


def rule(p, n, w, v):
    """The interior rule of include/hive_search.h, written out naively in float64 -> (edge, score)."""
    p, n, w = np.asarray(p, dtype=np.float64), np.asarray(n, dtype=np.int64), np.asarray(w, dtype=np.float64)
    if len(p) == 1:
        return 0, np.zeros(1)
    logit = np.log(np.maximum(p, 1e-30))
    sn = int(n.sum())
    q = [w[e] / n[e] if n[e] > 0 else None for e in range(len(p))]
    seen = [e for e in range(len(p)) if n[e] > 0]
    ps = sum(p[e] for e in seen)
    v_mix = v if sn == 0 or not ps > 0 else (v + sn * sum(p[e] * q[e] for e in seen) / ps) / (1 + sn)
    qc = np.array([v_mix if x is None else x for x in q])
    qn = (qc - qc.min()) / max(qc.max() - qc.min(), 1e-8)
    sigma = (C_VISIT + n.max()) * C_SCALE * qn
    z = np.exp(logit + sigma - (logit + sigma).max())
    score = z / z.sum() - n / (1.0 + sn)
    return int(np.argmax(score)), score


def puct(p, n, w):
    p, n, w = np.asarray(p, dtype=np.float64), np.asarray(n, dtype=np.int64), np.asarray(w, dtype=np.float64)
    q = np.where(n > 0, w / np.maximum(n, 1), 0.0)
    return int(np.argmax(q + C_PUCT * p * np.sqrt(n.sum() + 1) / (1 + n)))


def _both(p, n, w, v):
    """The restated rule and the package's statement of it must agree on the row."""
    edge, score = rule(p, n, w, v)
    got, got_score = mcts.gumbel_interior_choice(p, n, w, v)
    assert got == edge and np.abs(got_score - score).max() < 1e-12
    return edge


def test_rule_on_hand_made_rows():
    import hive_alphazero_amd.solo_play as sp
    assert sp.c_puct == C_PUCT and mcts.GUMBEL_DEFAULTS["c_visit"] == C_VISIT and mcts.GUMBEL_DEFAULTS["c_scale"] == C_SCALE
    zeros = lambda k: (np.zeros(k, dtype=np.int64), np.zeros(k))
    # nothing visited: sigma is flat, pi' is the priors and the choice is their argmax
    p = np.array([0.1, 0.2, 0.45, 0.25])
    for v in (-0.9, 0.0, 0.7):
        assert _both(p, *zeros(4), v) == 2
    rng = np.random.default_rng(5)
    for ne in (2, 35, 131, 256):
        p = rng.dirichlet(np.full(ne, 0.5))
        assert _both(p, *zeros(ne), 0.3) == int(np.argmax(p))
    # equal priors: the lower edge
    assert _both(np.full(5, 0.2), *zeros(5), 0.1) == 0
    n, w = np.array([1, 1, 0, 0, 0]), np.array([0.25, 0.25, 0.0, 0.0, 0.0])
    assert _both(np.full(5, 0.2), n, w, 0.25) == 2          # all q equal the mixed value: the first of the unvisited three
    # one visited child far above v_mix beats a higher prior; PUCT with the default c_puct follows the prior
    p = np.array([0.05, 0.9, 0.05])
    n, w = np.array([1, 0, 0]), np.array([-0.1, 0.0, 0.0])      # v = -0.8: v_mix = -0.45, the visited child's q = -0.1
    assert _both(p, n, w, -0.8) == 0
    assert puct(p, n, w) == 1                                   # q = 0 for the unvisited edges: the prior term decides
    # ... and a visited child far below it is left alone
    assert _both(p, np.array([0, 1, 0]), np.array([0.0, -0.9, 0.0]), 0.8) in (0, 2)
    # the pass edge: one edge with P = 0
    assert _both(np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1), 0.4) == 0
    assert _both(np.zeros(1), np.array([3]), np.array([-1.5]), 0.4) == 0
    # the visit share catches up: repeated selection with a fixed q spreads visits like pi'
    p = np.array([0.5, 0.3, 0.2])
    n, w = np.zeros(3, dtype=np.int64), np.zeros(3)
    for _ in range(40):
        e = _both(p, n, w, 0.0)
        n[e] += 1                                               # q stays 0 = v: pi' stays the priors
    assert np.abs(n - 40 * p).max() <= 1.0


# ------------------------------------------------------------------------------------------ option plumbing
def test_interior_needs_the_gumbel_root():
    opt = mcts.gumbel_interior_options
    assert opt(False, None) is False and opt(None, {"m": 16}) is False and opt(True, mcts.gumbel_options(True)) is True
    with pytest.raises(ValueError, match="gumbel_interior"):
        opt(True, None)
    # TreeSearch and ArenaSearch refuse it before they touch a device
    with pytest.raises(ValueError, match="gumbel_interior"):
        mcts.TreeSearch(4, 5, None, gumbel_interior=True)
    with pytest.raises(ValueError, match="gumbel_interior"):
        mcts.ArenaSearch(4, 5, None, None, None, gumbel_a=True, gumbel_interior_b=True)
    with pytest.raises(ValueError, match="per side"):
        mcts.ArenaSearch(4, 5, None, None, None, gumbel_a=True, gumbel_interior=True)
    # the pinned pieces of the root's options are what they were
    assert mcts.GUMBEL_DEFAULTS == {"m": 16, "c_visit": 50.0, "c_scale": 1.0}
    with pytest.raises(ValueError):
        mcts.gumbel_options({"interior": True})


def test_producer_hands_the_interior_key_to_its_children():
    from hive_alphazero_amd import self_play
    so = {"gumbel": True, "gumbel_interior": True}
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="compact", search_options=so)
    assert w.cfg["search_options"] == so and w.cfg["search_options"] is not so
    with pytest.raises(ValueError, match="gumbel_interior"):
        self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], search_options={"gumbel_interior": True})
    with pytest.raises(ValueError, match="one slot"):
        self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], slots=2, search_options=so)


# ------------------------------------------------------------------------------------------ ABI and header
def test_header_declares_the_calls_and_states_the_rule():
    from hive_alphazero_amd import _lib
    text = open(os.path.join(ROOT, "include", "hive_search.h")).read()
    for name in ("hive_search_set_gumbel_interior", "hive_search_node_values"):
        assert name + "(" in text and name in _lib.ABI_SYMBOLS, name
    flat = " ".join(text.split()).replace(" * ", " ")
    for words in ("score_e = pi'_e - (float)N_e / (1.0f + (float)SN)", "pi'_e = softmax_e(logit_e + sigma_e)",
                  "ties to the lower edge", "lifts that restriction", "no visit in flight", "ROOT ONLY"):
        assert words in flat, words
    assert flat.index("ROOT ONLY") < flat.index("lifts that restriction") < flat.index("int hive_search_set_gumbel(")
    assert flat.index("int hive_search_gumbel_fallbacks(") < flat.index("int hive_search_set_gumbel_interior(")
