"""The rules' numpy statements (hive_alphazero_amd/search_rules.py): the module needs neither torch nor the native library,
mcts re-exports every name, and rng_word -- the one statement of csrc/hive_rng.hpp's keying -- with the three draws built on
it gives, bit for bit, what the three hand-keyed statements it replaced gave.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hive_alphazero_amd import replay, search_rules
from hive_alphazero_amd.search_rules import gumbel_draw, playout_cap_draw, rng_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    """Draws recorded from replay.draw_indices, mcts.playout_cap_draw and mcts.gumbel_draw while each still keyed the
    generator by hand (64-bit values as hex strings)."""
    with open(os.path.join(ROOT, "tests", "golden", "search_rules_draws.json")) as f:
        return json.load(f)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _hex(values):
    return np.asarray([int(v, 16) for v in values], dtype=np.uint64)


def test_rules_and_sequential_player_import_without_torch():
    code = ("import sys; import hive_alphazero_amd.search_rules, hive_alphazero_amd.solo_play; "
            "assert 'torch' not in sys.modules, 'torch was imported'; "
            "assert 'hive_alphazero_amd.mcts' not in sys.modules, 'mcts was imported'")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_worker_options_are_checked_without_the_search_module():
    code = ("import sys; from hive_alphazero_amd.self_play import SelfPlayWorker\n"
            "try:\n"
            "    SelfPlayWorker(4, games_per_gpu=2, sims=10, gpus=[0], slots=3, search_options={'gumbel': True})\n"
            "except ValueError as e:\n"
            "    assert 'one slot only' in str(e), e\n"
            "else:\n"
            "    raise AssertionError('slots=3 with gumbel was accepted')\n"
            "assert 'hive_alphazero_amd.mcts' not in sys.modules and 'torch' not in sys.modules")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_mcts_keeps_every_moved_name():
    from hive_alphazero_amd import mcts
    moved = ["PUCT", "UCT", "LEAF_KINDS", "BUDGET_STREAM", "GUMBEL_STREAM", "GUMBEL_DEFAULTS", "full_threshold",
             "playout_cap_draw", "rolling_clock_step", "rolling_quantum", "rolling_options", "gumbel_considered_visits",
             "gumbel_draw", "gumbel_improved_policy", "gumbel_options", "gumbel_interior_options", "gumbel_interior_choice"]
    assert set(moved) | {"rng_word"} == set(search_rules.__all__)
    for name in search_rules.__all__:
        assert getattr(mcts, name) is getattr(search_rules, name), name
    assert replay._splitmix is search_rules._splitmix and replay._M64 == search_rules._M64 == 2 ** 64 - 1


def test_rng_word_pinned():
    assert int(rng_word(0, 0, 0, 0)) == 0x2130748AAAC80268
    assert int(rng_word(1, 2, 3, 4)) == 0x3BDFC869CEC2FF10
    assert int(rng_word(2 ** 64 - 1, 2 ** 63, 2 ** 40, 255)) == 0x798CCCBEBF9A09B0


def test_rng_word_type_and_broadcast():
    one = rng_word(1, 2, 3, 4)
    assert isinstance(one, np.ndarray) and one.dtype == np.uint64 and one.shape == ()
    a, c = np.arange(3, dtype=np.int64)[:, None], np.arange(5, dtype=np.uint64)
    grid = rng_word(7, a, 2 ** 70 + 9, c)                        # keys are taken mod 2^64
    assert grid.dtype == np.uint64 and grid.shape == (3, 5)
    for i in range(3):
        for j in range(5):
            assert grid[i, j] == rng_word(7, i, 9, j)
    assert rng_word(0, np.int64(-1), 0, 0) == rng_word(0, 2 ** 64 - 1, 0, 0)      # int64 wraps as the device's cast does
    assert rng_word(-1, 0, 0, 0) == rng_word(2 ** 64 - 1, 0, 0, 0)


def test_draw_indices_pinned():
    assert replay.draw_indices(9, 4, 2, 6, 1000).tolist() == [266, 685, 120, 525, 917, 903]
    assert replay.draw_indices(2 ** 64 - 3, 123456789, 7, 5, 2 ** 32 - 1).tolist() == \
        [607163723, 7587161, 1253476113, 2785229845, 720797918]


def test_playout_cap_draw_pinned():
    got = playout_cap_draw(7, np.arange(8) + 100, np.arange(8) + 1, 0.25)
    assert got.dtype == bool and got.astype(int).tolist() == [0, 0, 1, 0, 1, 0, 1, 0]


def test_gumbel_draw_pinned():
    assert np.array_equal(_bits(gumbel_draw(5, 11, 9, 4)),
                          _hex(["0x400524BCEDB410E1", "0xBFF3F93AD2CBD709", "0x3FE43F319F5A11CD", "0xBFC17B99C5ABDDDC"]))
    assert np.array_equal(_bits(gumbel_draw(2 ** 64 - 1, 2 ** 40 + 3, 54, 3)),
                          _hex(["0x3FE185375B1047B2", "0xBFD5D61488F6AC63", "0x3FE503F3EEF118F7"]))
    assert np.array_equal(gumbel_draw(5, 11, 9, 4, quiet=True), np.zeros(4))


def test_recorded_draws(recorded):
    assert len(recorded["rng_word"]) >= 24 and len(recorded["draw_indices"]) >= 12
    assert len(recorded["playout_cap_draw"]) >= 10 and len(recorded["gumbel_draw"]) >= 12
    for case in recorded["rng_word"]:
        got = rng_word(*[int(k, 16) for k in case["key"]])
        assert np.array_equal(got.reshape(1), _hex([case["word"]])), case
    for case in recorded["draw_indices"]:
        got = replay.draw_indices(int(case["seed"], 16), case["step"], case["stream_id"], case["n"], case["live"])
        assert got.dtype == np.int64 and np.array_equal(got, np.asarray(case["rows"], dtype=np.int64)), case
    for case in recorded["playout_cap_draw"]:
        got = playout_cap_draw(int(case["seed"], 16), case["game_ids"], case["turns"], case["p_full"])
        assert got.dtype == bool and np.array_equal(got, np.asarray(case["full"], dtype=bool)), case
    for case in recorded["gumbel_draw"]:
        got = gumbel_draw(int(case["seed"], 16), case["game_id"], case["turn"], case["ne"])
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _hex(case["bits"])), case
