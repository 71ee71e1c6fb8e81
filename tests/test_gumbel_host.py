"""The Gumbel root with sequential halving, host side (no GPU): the schedule against the paper's loop, the law and purity of
the draws, the improved policy, the sequential statement (solo_play.HivePlayer.gumbel) on the CPU oracle env, the options
parser with every refusal, and the ABI's declarations."""
import math
import os

import numpy as np
import pytest

from hive_alphazero_amd import mcts
from mcts_stub import StubPipe
from oracle_env import OracleGamePlay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(m, n) for m in range(1, 33) for n in range(1, 71)] + [(16, 199), (256, 255)]


def paper_sequence(m, n):
    """get_sequence_of_considered_visits of the published algorithm, restated naively."""
    if m <= 1:
        return list(range(n))
    log2max = int(math.ceil(math.log2(m)))
    sequence, visits, considered = [], [0] * m, m
    while len(sequence) < n:
        extra = max(1, int(n / (log2max * considered)))
        for _ in range(extra):
            sequence.extend(visits[:considered])
            for i in range(considered):
                visits[i] += 1
        considered = max(2, considered // 2)
    return sequence[:n]


def test_schedule_equals_the_papers_loop():
    for m, n in GRID:
        got = mcts.gumbel_considered_visits(m, n)
        assert got.dtype == np.int32 and got.tolist() == paper_sequence(m, n), (m, n)
    assert mcts.gumbel_considered_visits(16, 32).tolist() == [0] * 16 + [1] * 8 + [2, 2, 2, 2, 3, 3, 3, 3]
    for m, n in ((16, 15), (8, 3), (32, 31), (2, 1)):
        assert not mcts.gumbel_considered_visits(m, n).any(), (m, n)
    assert mcts.gumbel_considered_visits(1, 5).tolist() == [0, 1, 2, 3, 4]
    assert mcts.gumbel_considered_visits(16, 0).tolist() == []


def test_draws_follow_the_gumbel_law_and_are_pure():
    """100,000 draws (1000 roots x 100 edges).  A standard Gumbel has mean 0.57722 and variance pi^2 / 6; the mean of n draws
    has standard deviation sqrt(pi^2 / 6 / n), the sample variance sqrt((mu4 - var^2) / n) with mu4 = 5.4 var^2 (kurtosis
    5.4).  Both are held to 5 of those."""
    roots, ne = 1000, 100
    g = np.concatenate([mcts.gumbel_draw(20260, 7000 + r // 40, r % 40 + 1, ne) for r in range(roots)])
    n, var = g.size, math.pi ** 2 / 6
    assert n == 100_000 and g.dtype == np.float64 and np.isfinite(g).all()
    print(f"mean {g.mean():.5f} variance {g.var():.5f}")
    assert abs(g.mean() - 0.57722) <= 5 * math.sqrt(var / n)
    assert abs(g.var() - var) <= 5 * math.sqrt(4.4 * var * var / n)
    # a pure function of its keys: the same keys give the same bits, each key matters, a prefix of the edges is a prefix
    a = mcts.gumbel_draw(5, 11, 9, 131)
    assert np.array_equal(a.view(np.uint64), mcts.gumbel_draw(5, 11, 9, 131).view(np.uint64))
    assert np.array_equal(a[:35], mcts.gumbel_draw(5, 11, 9, 35))
    for other in ((6, 11, 9), (5, 12, 9), (5, 11, 10)):
        assert not np.array_equal(a, mcts.gumbel_draw(*other, 131))
    quiet = mcts.gumbel_draw(5, 11, 9, 131, quiet=True)
    assert quiet.shape == (131,) and not quiet.any()
    assert isinstance(mcts.GUMBEL_STREAM, int) and mcts.GUMBEL_STREAM != mcts.BUDGET_STREAM


def test_improved_policy():
    rng = np.random.default_rng(1)
    for ne in (1, 2, 35, 131):
        p = rng.dirichlet(np.full(ne, 0.5)).astype(np.float32)
        n = rng.integers(0, 5, ne)
        w = np.where(n > 0, rng.uniform(-1, 1, ne) * n, 0.0)
        score, improved = mcts.gumbel_improved_policy(p, n, w, 0.3, 50.0, 1.0)
        assert score.shape == improved.shape == (ne,) and abs(improved.sum() - 1.0) < 1e-6 and (improved > 0).all()
        # without visits every completed q is v_root: sigma = 0 and the improved policy is the priors
        score0, prior = mcts.gumbel_improved_policy(p, np.zeros(ne, dtype=int), np.zeros(ne), -0.7, 50.0, 1.0)
        assert np.abs(prior - p / p.sum()).max() < 1e-6
        assert np.allclose(score0, np.log(np.maximum(p.astype(np.float64), 1e-30)))
    # raising one visited edge's W raises that edge's probability
    p = rng.dirichlet(np.full(20, 0.5))
    n = np.array([3, 0, 1, 2, 0] * 4)
    w = np.where(n > 0, rng.uniform(-0.5, 0.5, 20) * n, 0.0)
    before = mcts.gumbel_improved_policy(p, n, w, 0.1)[1]
    for e in np.flatnonzero(n > 0):
        w2 = w.copy()
        w2[e] += 0.4 * n[e]
        assert mcts.gumbel_improved_policy(p, n, w2, 0.1)[1][e] > before[e], e
    # the defaults are the paper's
    assert mcts.GUMBEL_DEFAULTS == {"m": 16, "c_visit": 50.0, "c_scale": 1.0}
    assert np.array_equal(before, mcts.gumbel_improved_policy(p, n, w, 0.1, 50.0, 1.0)[1])


def _position(prefix_seed, plies):
    rng = np.random.default_rng(prefix_seed)
    g = OracleGamePlay()
    for _ in range(plies):
        acts = g.actions()
        g.move(int(acts[rng.integers(len(acts))]))
    return g


@pytest.mark.parametrize("prefix_seed,plies,noisy", [(21, 0, True), (22, 3, True), (23, 8, False), (24, 14, True)])
def test_sequential_mirror_spends_its_visits_by_the_schedule(prefix_seed, plies, noisy):
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    assert sp.HivePlayer.gumbel is None
    sims, M = 33, 16
    g = _position(prefix_seed, plies)
    ne = len(g.actions())
    player = sp.HivePlayer(pipes=[StubPipe()])
    player.simulation_num_per_move = sims
    draw = (lambda turn, k: mcts.gumbel_draw(77, 5, turn, k)) if noisy else None
    player.gumbel = {"m": M, "g": draw}
    state = np.random.get_state()
    move, (policy, visits) = player.action(g)
    assert np.array_equal(state[1], np.random.get_state()[1])      # no Dirichlet noise, no sampled move: numpy's stream is untouched
    root = player.tree[g.state_key]
    counts = sorted(e.n for e in root.a.values())
    sched = mcts.gumbel_considered_visits(min(M, ne), sims - 1)
    # the multiset the schedule implies: slot j of the considered actions is visited once per entry that exceeds ... i.e.
    # replay the schedule on anonymous slots -- every entry t moves one slot from t to t + 1 visits
    slots = [0] * ne
    for t in sched.tolist():
        slots[slots.index(t)] += 1
    assert player.gumbel_fallbacks == 0 and int(visits) == sims - 1 == root.sum_n
    assert counts == sorted(slots)
    if ne >= 16:
        assert [c for c in counts if c] == [1] * 8 + [2] * 4 + [4] * 4
    most = max(counts)
    assert move in g.actions() and root.a[move].n == most
    policy = np.asarray(policy)
    assert abs(policy.sum() - 1.0) < 1e-6 and set(np.flatnonzero(policy)) == set(g.actions())
    assert player.gumbel_min_gap > 0
    if not noisy:                                                   # g = 0: the same search twice
        again = sp.HivePlayer(pipes=[StubPipe()])
        again.simulation_num_per_move = sims
        again.gumbel = {"m": M}
        assert again.action(g)[0] == move


def test_mirror_with_one_simulation_answers_with_the_priors():
    import hive_alphazero_amd.solo_play as sp
    sp.SEARCH_THREADS = 1
    g = _position(22, 3)
    acts = g.actions()
    gd = mcts.gumbel_draw(3, 4, g.state.turn, len(acts))
    player = sp.HivePlayer(pipes=[StubPipe()])
    player.simulation_num_per_move = 1
    player.gumbel = {"g": gd}
    move, (policy, visits) = player.action(g)
    p = np.array([float(player.tree[g.state_key].a[a].p) for a in acts])
    assert visits == 0 and np.abs(np.asarray(policy)[acts] - p / p.sum()).max() < 1e-6
    assert move == acts[int(np.argmax(gd + np.log(p)))]


def test_options_parser_accepts_and_refuses():
    opt = mcts.gumbel_options
    for off in (None, False, 0, {}):
        assert opt(off) is None
        assert opt(off, slots=4, mode=mcts.UCT, keep_tree=True) is None       # off: nothing to refuse
    assert opt(True) == {"m": 16, "c_visit": 50.0, "c_scale": 1.0} == mcts.GUMBEL_DEFAULTS
    assert opt({"m": 8}) == {"m": 8, "c_visit": 50.0, "c_scale": 1.0}
    given = {"m": 4, "c_visit": 30, "c_scale": 0.5}
    got = opt(given, 1, mcts.PUCT, False)
    assert got == {"m": 4, "c_visit": 30.0, "c_scale": 0.5} and got is not given
    assert opt(got) == got                                                   # a parsed option parses to itself
    for bad in ({"sims": 3}, {"m": 0}, {"m": 16, "c_visit": -1.0}, {"m": 16, "c_scale": 0.0}, {"c_visit": float("nan")}):
        with pytest.raises(ValueError):
            opt(bad)
    with pytest.raises(ValueError, match="one slot"):
        opt(True, slots=2)
    with pytest.raises(ValueError, match="UCT"):
        opt(True, mode=mcts.UCT)
    with pytest.raises(ValueError, match="keep_tree"):
        opt({"m": 8}, keep_tree=True)


def test_producer_hands_search_options_to_its_children():
    from hive_alphazero_amd import self_play
    so = {"gumbel": {"m": 8}}
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="compact", rolling=True, search_options=so)
    assert w.cfg["search_options"] == so and w.cfg["search_options"] is not so
    assert self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0]).cfg["search_options"] is None
    with pytest.raises(ValueError, match="one slot"):
        self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], slots=2, search_options={"gumbel": True})
    with pytest.raises(ValueError, match="keep_tree"):
        self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], search_options={"gumbel": True, "keep_tree": True})


def test_header_declares_the_calls_and_says_what_is_refused():
    from hive_alphazero_amd import _lib
    text = open(os.path.join(ROOT, "include", "hive_search.h")).read()
    for name in ("hive_search_set_gumbel", "hive_search_gumbel_schedule", "hive_search_root_gumbel",
                 "hive_search_gumbel_fallbacks"):
        assert name + "(" in text and name in _lib.ABI_SYMBOLS, name
    flat = " ".join(text.split())
    for words in ("slots > 1", "UCT mode", "hive_search_advance_roots returns HIVE_E_ARG while on", "ROOT ONLY",
                  "have not been tuned"):
        assert words in flat.replace(" * ", " "), words
    assert f"0x{mcts.GUMBEL_STREAM:016X}" in text
    assert _lib.ctypes.sizeof(mcts._GumbelParams) == 16
