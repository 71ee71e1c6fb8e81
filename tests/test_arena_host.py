"""Arena, host side (no GPU): the match statistics against values worked out by hand, the game-id -> (pair, colour)
mapping, and a pure-Python mirror of the opening draw of hive_arena_opening_launch (used by tests/test_gpu_arena.py)."""
import math

import pytest

from hive_alphazero_amd import arena
from hive_alphazero_amd.arena import A_WIN, B_WIN, CAP, DRAW, ArenaResult

M64 = (1 << 64) - 1


# ---- the counter-based generator of csrc/hive_rng.hpp in 64-bit masked integers
def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_state(seed, a, b, c):
    inner = splitmix((b * 0x9E3779B1 + c) & M64)
    return splitmix((seed & M64) ^ splitmix((a * 0x100000001B3 + inner) & M64))


def opening_index(seed, pair, turn, count):
    """Index into the ascending legal-id list that hive_arena_opening_launch picks for (seed, pair, turn)."""
    r = splitmix(rng_state(seed, pair & M64, turn, 0))
    return ((r >> 32) * count) >> 32


def opening_action(seed, pair, turn, legal):
    return legal[opening_index(seed, pair, turn, len(legal))] if legal else -1


def _result(codes):
    """ArenaResult of the games {game id: code} (every game 30 turns long)."""
    tally = [0] * 8
    for g, c in codes.items():
        a_white = g % 2 == 0
        if c == A_WIN:
            tally[0 if a_white else 1] += 1
        elif c == B_WIN:
            tally[3 if a_white else 2] += 1
        else:
            tally[4 if c == DRAW else 5] += 1
        tally[6] += 1
        tally[7] += 30
    return ArenaResult(tally, arena.pair_scores(codes))


def test_mirror_is_a_64_bit_generator():
    # splitmix64's first output for the state 0 (the published test vector of the generator)
    assert splitmix(0) == 0xE220A8397B1DCDAF
    seen = {opening_index(7, pair, turn, 40) for pair in range(64) for turn in range(1, 5)}
    assert all(0 <= i < 40 for i in seen) and len(seen) > 30
    assert opening_index(7, 3, 2, 40) == opening_index(7, 3, 2, 40)
    assert [opening_index(7, 3, t, 1) for t in range(1, 5)] == [0, 0, 0, 0]
    assert opening_action(7, 3, 2, []) == -1


def test_game_ids_map_to_pair_and_colour():
    assert arena.game_pair(0) == (0, True) and arena.game_pair(1) == (0, False)
    assert arena.game_pair(10) == (5, True) and arena.game_pair(11) == (5, False)
    for k in (0, 1, 17, 4095):
        w, b = arena.pair_games(k)
        assert arena.game_pair(w) == (k, True) and arena.game_pair(b) == (k, False)
    assert list(arena.game_ids_of_pairs([3, 0, 8])) == [6, 7, 0, 1, 16, 17]
    assert list(arena.game_ids_of_pairs(range(2))) == [0, 1, 2, 3]


def test_all_wins_and_all_losses_have_a_finite_clipped_elo():
    n = 20
    win = _result({g: A_WIN for g in range(n)})
    assert (win.wins, win.losses, win.draws, win.caps, win.games) == (20, 0, 0, 0, 20)
    assert (win.a_wins_white, win.a_wins_black) == (10, 10)
    assert win.score == 1.0 and win.pair_scores == [1.0] * 10 and win.se == 0.0
    # clipped by half a game: 1 - 1/40 = 0.975 -> 400 log10(0.975 / 0.025) = 400 log10(39)
    assert win.elo == pytest.approx(400.0 * math.log10(39.0), abs=1e-9) and math.isfinite(win.elo)
    assert win.elo == pytest.approx(636.43, abs=0.01)
    assert win.score_ci95 == (0.975, 0.975) and all(math.isfinite(e) for e in win.elo_ci95)
    assert win.passes() and win.passes_ci()
    loss = _result({g: B_WIN for g in range(n)})
    assert (loss.wins, loss.losses, loss.b_wins_white, loss.b_wins_black) == (0, 20, 10, 10)
    assert loss.score == 0.0 and loss.elo == pytest.approx(-400.0 * math.log10(39.0), abs=1e-9)
    assert not loss.passes() and not loss.passes_ci()
    assert loss.mean_game_length == 29.0


def test_ten_win_loss_pairs_score_one_half_with_zero_variance():
    codes = {}
    for k in range(10):
        codes[2 * k], codes[2 * k + 1] = A_WIN, B_WIN          # white wins both games of every pair
    r = _result(codes)
    assert (r.a_wins_white, r.a_wins_black, r.b_wins_white, r.b_wins_black) == (10, 0, 10, 0)
    assert r.score == 0.5 and r.pair_scores == [0.5] * 10 and r.se == 0.0
    assert r.elo == 0.0 and r.score_ci95 == (0.5, 0.5) and r.elo_ci95 == (0.0, 0.0)
    assert not r.passes() and not r.passes_ci()


def test_mixed_match_has_the_pentanomial_standard_error():
    # 4 pairs: (win, win) (win, draw) (loss, cap) (win, loss) -> x = 1, .75, .25, .5
    codes = {0: A_WIN, 1: A_WIN, 2: A_WIN, 3: DRAW, 4: B_WIN, 5: CAP, 6: A_WIN, 7: B_WIN}
    r = _result(codes)
    assert r.pair_scores == [1.0, 0.75, 0.25, 0.5]
    assert (r.wins, r.losses, r.draws, r.caps) == (4, 2, 1, 1)
    assert (r.a_wins_white, r.a_wins_black, r.b_wins_white, r.b_wins_black) == (3, 1, 1, 1)
    # score = (4 + 2 / 2) / 8 = 0.625 = mean(x); deviations .375 .125 -.375 -.125 -> sum of squares .3125;
    # var(ddof=1) = .3125 / 3; se = sqrt(.3125 / 3 / 4) = sqrt(.0260416...) = 0.161374...
    assert r.score == 0.625
    assert r.se == pytest.approx(math.sqrt(0.3125 / 12.0), abs=1e-12) and r.se == pytest.approx(0.1613743, abs=1e-6)
    lo, hi = 0.625 - 1.96 * r.se, 0.625 + 1.96 * r.se          # 0.30871 .. 0.94129
    assert r.score_ci95 == pytest.approx((lo, min(hi, 1 - 1 / 16)), abs=1e-12)
    assert r.elo == pytest.approx(-400.0 * math.log10(1 / 0.625 - 1), abs=1e-9) and r.elo == pytest.approx(88.74, abs=0.01)
    assert r.elo_ci95[0] == pytest.approx(-400.0 * math.log10(1 / lo - 1), abs=1e-9) and r.elo_ci95[0] < 0 < r.elo_ci95[1]
    assert r.passes() and not r.passes_ci()
    # an incomplete pair does not enter the paired statistics
    assert arena.pair_scores({0: A_WIN, 1: B_WIN, 2: A_WIN}) == [0.5]
    assert arena.pentanomial_se([0.5]) == math.inf


def test_gates_on_both_sides_of_their_thresholds():
    def match(wins, pairs=50):
        """`wins` pairs won outright (both games), the rest split."""
        codes = {}
        for k in range(pairs):
            codes[2 * k] = A_WIN
            codes[2 * k + 1] = A_WIN if k < wins else B_WIN
        return _result(codes)
    r = match(5)                                                 # score (50 + 5) / 100 = 0.55
    assert r.score == 0.55 and r.passes() and not r.passes(0.56)
    r = match(4)                                                 # 0.54
    assert r.score == 0.54 and not r.passes() and r.passes(0.54)
    # x = 1 (w times) and .5 (50 - w times): mean .5 + w / 100, var(ddof=1) = .25 w (50 - w) / (50 * 49)
    for w, expect in ((3, False), (4, True)):
        r = match(w)
        se = math.sqrt(0.25 * w * (50 - w) / (50 * 49) / 50)
        assert r.se == pytest.approx(se, abs=1e-12)
        assert (0.5 + w / 100 - 1.96 * se > 0.5) == expect       # w = 3: 0.4968, w = 4: 0.5020
        assert r.passes_ci() == expect
    empty = ArenaResult([0] * 8, [])
    assert not empty.passes() and not empty.passes_ci() and empty.mean_game_length == 0.0


def test_arena_symbols_are_declared():
    from hive_alphazero_amd import _lib
    for name in ("hive_arena_split_launch", "hive_arena_join_launch", "hive_arena_opening_launch", "hive_arena_score_launch"):
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(_lib.load(), name)
