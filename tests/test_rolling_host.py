"""Rolling search on the host: the per-game clock rule (mcts.rolling_clock_step) against a table written by hand and against
the layout TreeSearch.run_simulations gives a search, the new ABI symbols, and the producer's options.  No GPU."""
import os
import re

import numpy as np
import pytest

from hive_alphazero_amd import mcts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hive_search_set_rolling", "hive_search_round_end", "hive_search_restart", "hive_search_policy_where",
               "hive_search_clocks")

# budgets of the six games; the last one is inactive
BUDGET = [0, 1, 2, 5, 8, 5]
ACTIVE = [1, 1, 1, 1, 1, 0]
# per slot count: the rounds, each a row per game of the slots it runs ("x" = takes part), and the round (1-based) after which
# each game is done (0 = never: the inactive game)
TABLE = {
    1: {"rounds": [["-", "x", "x", "x", "x", "-"],
                   ["-", "-", "x", "x", "x", "-"],
                   ["-", "-", "-", "x", "x", "-"],
                   ["-", "-", "-", "x", "x", "-"],
                   ["-", "-", "-", "x", "x", "-"],
                   ["-", "-", "-", "-", "x", "-"],
                   ["-", "-", "-", "-", "x", "-"],
                   ["-", "-", "-", "-", "x", "-"],
                   ["-", "-", "-", "-", "-", "-"]],
        "done_after": [1, 1, 2, 5, 8, 0]},
    3: {"rounds": [["---", "x--", "x--", "x--", "x--", "---"],       # the root-opening simulation runs alone
                   ["---", "---", "x--", "xxx", "xxx", "---"],       # simulations 1, 2, 3
                   ["---", "---", "---", "x--", "xxx", "---"],       # budget 5: simulation 4 alone; budget 8: 4, 5, 6
                   ["---", "---", "---", "---", "x--", "---"],       # budget 8: simulation 7
                   ["---", "---", "---", "---", "---", "---"]],
        "done_after": [1, 1, 2, 3, 4, 0]},
}


@pytest.mark.parametrize("slots", [1, 3])
def test_clock_step_equals_the_hand_written_table(slots):
    want = TABLE[slots]
    clock = np.zeros(len(BUDGET), dtype=np.int64)
    first_done = [0] * len(BUDGET)
    for r, row in enumerate(want["rounds"], start=1):
        part, clock, done = mcts.rolling_clock_step(clock, BUDGET, ACTIVE, slots)
        assert part.shape == (len(BUDGET), slots) and part.dtype == bool
        got = ["".join("x" if x else "-" for x in g) for g in part]
        assert got == row, (slots, r)
        for g, d in enumerate(done):
            if d and not first_done[g]:
                first_done[g] = r
            assert bool(d) == bool(first_done[g]), (slots, r, g)         # done stays done
    assert first_done == want["done_after"]
    assert clock.tolist() == [0, 1, 2, 5, 8, 0]                           # a clock ends at its budget; the idle one never moves


def _run_simulations_layout(sims, slots):
    """[(simulation number, slot)] round by round, as TreeSearch.run_simulations lays a search of `sims` out: its loop, with
    the host counter hive_search_select increments."""
    rounds, done, first, counter = [], 0, True, 0
    while done < sims:
        k = 1 if first else min(slots, sims - done)
        rounds.append([(counter + sl, sl) for sl in range(k)])
        counter += k
        done += k
        first = False
    return rounds


@pytest.mark.parametrize("slots", [1, 2, 3, 8])
def test_a_game_runs_the_simulations_a_lock_step_search_of_its_budget_runs(slots):
    budgets = np.arange(0, 41)
    clock = np.zeros(len(budgets), dtype=np.int64)
    got = [[] for _ in budgets]
    rounds_to_done = np.zeros(len(budgets), dtype=np.int64)
    for r in range(1, 45):
        part, after, done = mcts.rolling_clock_step(clock, budgets, np.ones(len(budgets)), slots)
        for g in range(len(budgets)):
            pairs = [(int(clock[g]) + sl, sl) for sl in range(slots) if part[g, sl]]
            if pairs:
                got[g].append(pairs)
        rounds_to_done[(rounds_to_done == 0) & done] = r
        clock = after
    for g, b in enumerate(budgets.tolist()):
        assert got[g] == _run_simulations_layout(b, slots), (slots, b)
        assert clock[g] == b
        if b >= 1:
            assert rounds_to_done[g] == mcts.rolling_quantum(b, slots) == len(got[g]), (slots, b)
    assert mcts.rolling_quantum(10, 1) == 10 and mcts.rolling_quantum(50, 1) == 50 and mcts.rolling_quantum(8, 3) == 4


def test_new_symbols_are_declared_exported_and_bound():
    from hive_alphazero_amd import _lib
    text = open(os.path.join(ROOT, "include", "hive_search.h")).read()
    declared = set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(hive_\w+)\s*\(", text, re.M))
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.ABI_SYMBOLS, name
        assert getattr(L, name).argtypes, name


def test_producer_hands_the_options_to_its_children():
    from hive_alphazero_amd import self_play
    cap = {"full": 50, "fast": 10, "p_full": 0.25}
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="compact", playout_cap=cap, rolling={"quantum": 3})
    assert w.cfg["playout_cap"] == cap and w.cfg["rolling"] == {"quantum": 3}
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="compact", rolling=True)
    assert w.cfg["rolling"] is True and w.cfg["playout_cap"] is None
    w = self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0])
    assert w.cfg["rolling"] is None and w.cfg["playout_cap"] is None
    for kw in ({"playout_cap": cap}, {"rolling": True}, {"playout_cap": cap, "rolling": True}):
        with pytest.raises(ValueError):
            self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], row_format="json", **kw)
        with pytest.raises(ValueError):
            self_play.SelfPlayWorker(8, games_per_gpu=4, gpus=[0], **kw)      # json is the default
    assert "rolling" in self_play.SelfPlayWorker.__doc__
