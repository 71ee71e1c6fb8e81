"""Arena: two networks play a match on one GPU (woker/evaluation.py:40-111,128-310 for every game at once).

`pairs` pairs of games are played in lock step.  The two games of a pair start from the same uniformly random opening
(evaluation.py:169,187: random moves while turn <= 4) with the colours swapped, the side to move always searches with its
own network (mcts.ArenaSearch), moves are the argmax of the visit counts (the reference's temperature), and the result is
the tally of hive_arena_score_launch with the paired-game statistics below.

Game ids: game 2k is pair k with A as white, game 2k + 1 is pair k with B as white.  The search's game ids are these
global ids and the opening is keyed on (seed, pair, turn), so a game's moves depend on (seed, game id) only -- not on the
slot, `games_in_flight` or the order in which other games retire.

The statistics (`pair_scores`, `score_interval`, `elo`, `ArenaResult`) are plain Python and need no GPU.
"""
import ctypes
import math

from ._lib import ptr as _p, stream_ptr
from .config import MAX_GAME_LENGTH

A_WIN, B_WIN, DRAW, CAP = 1, 2, 3, 4                 # result codes of hive_arena_score_launch
MAX_MOVES = MAX_GAME_LENGTH - 1                      # a game is capped when its turn reaches MAX_GAME_LENGTH
TALLY = ("a_wins_white", "a_wins_black", "b_wins_white", "b_wins_black", "draws", "caps", "games", "turn_sum")


# ---------------------------------------------------------------------------------------- ids
def game_pair(game_id):
    """Global game id -> (pair index, A plays white)."""
    return int(game_id) // 2, int(game_id) % 2 == 0


def pair_games(pair):
    """Pair index -> (game id with A as white, game id with B as white)."""
    return 2 * int(pair), 2 * int(pair) + 1


def game_ids_of_pairs(pair_ids):
    """The game-id stream of a pair-id stream: both games of a pair, A-as-white first."""
    for k in pair_ids:
        yield 2 * int(k)
        yield 2 * int(k) + 1


# ---------------------------------------------------------------------------------------- statistics
def game_score(result):
    """A's score of one game: 1 win, 0 loss, 1/2 draw or length cap."""
    return {A_WIN: 1.0, B_WIN: 0.0, DRAW: 0.5, CAP: 0.5}[int(result)]


def pair_scores(results):
    """{game id: result code} -> the mean score x_k of every COMPLETE pair, by ascending pair index (values in
    {0, .25, .5, .75, 1}: the pentanomial outcome of a pair of games from one opening with the colours swapped)."""
    out = []
    for k in sorted({int(g) // 2 for g in results}):
        w, b = pair_games(k)
        if w in results and b in results:
            out.append(0.5 * (game_score(results[w]) + game_score(results[b])))
    return out


def pentanomial_se(x):
    """Standard error of the match score from the per-pair means: sqrt(var(x, ddof=1) / pairs).  The two games of a pair
    share their opening, so they are not independent; the pairs are.  Fewer than two pairs: infinite."""
    n = len(x)
    if n < 2:
        return math.inf
    m = sum(x) / n
    return math.sqrt(sum((v - m) ** 2 for v in x) / (n - 1) / n)


def clip_score(score, games):
    """A score clipped into (0, 1) by half a game, [1 / 2N, 1 - 1 / 2N]: what an all-wins match of N games can claim."""
    eps = 0.5 / max(int(games), 1)
    return min(max(float(score), eps), 1.0 - eps)


def elo(score, games):
    """-400 log10(1 / score - 1), the score clipped by half a game first (finite for 0 and 1)."""
    s = clip_score(score, games)
    return -400.0 * math.log10(1.0 / s - 1.0) + 0.0      # (+ 0.0: an even score reads 0.0, not -0.0)


def score_interval(score, x):
    """score +- 1.96 se of the per-pair means x (unclipped; (-inf, inf) with fewer than two pairs)."""
    half = 1.96 * pentanomial_se(x)
    return score - half, score + half


class ArenaResult:
    """A match from network A's point of view.  Built from the eight counters of hive_arena_score_launch and the per-pair
    mean scores."""

    def __init__(self, tally, pairs_x):
        t = [int(v) for v in tally]
        assert len(t) == 8
        for name, v in zip(TALLY, t):
            setattr(self, name, v)
        self.pair_scores = [float(v) for v in pairs_x]
        self.wins, self.losses = self.a_wins_white + self.a_wins_black, self.b_wins_white + self.b_wins_black
        assert self.wins + self.losses + self.draws + self.caps == self.games
        n = max(self.games, 1)
        self.score = (self.wins + 0.5 * (self.draws + self.caps)) / n
        self.elo = elo(self.score, n)
        self.se = pentanomial_se(self.pair_scores)
        lo, hi = score_interval(self.score, self.pair_scores)
        self.score_ci95 = (clip_score(lo, n), clip_score(hi, n))
        self.elo_ci95 = (elo(lo, n), elo(hi, n))
        # plies of the finished games = final turn number - 1 (as mcts.SelfPlay.mean_game_length)
        self.mean_game_length = self.turn_sum / n - 1.0 if self.games else 0.0

    def passes(self, min_score=0.55):
        """AlphaZero's gate: the candidate (A) scored at least min_score."""
        return self.games > 0 and self.score >= min_score

    def passes_ci(self):
        """The lower end of the 95 % interval of the score is above 1/2."""
        return self.games > 0 and self.score_ci95[0] > 0.5

    def as_dict(self):
        d = {k: getattr(self, k) for k in TALLY[:7]}
        d.update(wins=self.wins, losses=self.losses, pairs=len(self.pair_scores), score=self.score, elo=self.elo,
                 score_ci95=list(self.score_ci95), elo_ci95=list(self.elo_ci95), mean_game_length=self.mean_game_length)
        return d

    def __repr__(self):
        return (f"ArenaResult(A {self.wins} wins ({self.a_wins_white} as white, {self.a_wins_black} as black), "
                f"B {self.losses} wins ({self.b_wins_white} as white, {self.b_wins_black} as black), {self.draws} draws, "
                f"{self.caps} at the length cap; {self.games} games in {len(self.pair_scores)} pairs, mean length "
                f"{self.mean_game_length:.1f} plies; score {self.score:.3f} [{self.score_ci95[0]:.3f}, {self.score_ci95[1]:.3f}], "
                f"elo {self.elo:+.0f} [{self.elo_ci95[0]:+.0f}, {self.elo_ci95[1]:+.0f}])")


# ---------------------------------------------------------------------------------------- the engine
class Arena:
    """`pairs` pairs of games between evaluator_a and evaluator_b, `games_in_flight` of them in lock step.

    arena.run() -> ArenaResult, or `while arena.running(): arena.play_ply()` and `arena.result()`.
    arena.games[game_id] = (result code, [moves]) for every finished game (keep_moves), arena.results[game_id] = code.

    sims_b (default None: both sides search `sims` simulations): the sides search unequally, A with `sims` and B with
    `sims_b` simulations per move.  The batch then runs max(sims, sims_b) simulations and every game drops out of it after
    its owner's share (hive_arena_budget_launch at every ply + the search's per-game budgets); rows_evaluated() shows what
    each side cost.  The first use: how much stronger is one network with 50 simulations than with 10.

    gumbel_a / gumbel_b (None | True | {"m", "c_visit", "c_scale"}): that side searches with the Gumbel root and plays
    argmax(g + logit + sigma(q)) (mcts.ArenaSearch); the other side's searches are untouched.
    gumbel_interior_a / gumbel_interior_b: that side's Gumbel searches also use the Gumbel rule below the root; it needs
    the side's gumbel_*.  gumbel_a=True, gumbel_b=True, gumbel_interior_a=True: full Gumbel against root-only Gumbel.
    solver_a / solver_b: that side searches with proven wins and losses below the root (mcts.ArenaSearch); not in a match
    where either side has the Gumbel root."""

    def __init__(self, evaluator_a, evaluator_b, pairs=512, sims=50, slots=1, games_in_flight=1024, seed=0, opening_turns=4,
                 noise_eps=0.0, pair_ids=None, keep_moves=True, device=None, search_options=None, sims_b=None,
                 gumbel_a=None, gumbel_b=None, gumbel_interior_a=False, gumbel_interior_b=False, solver_a=False,
                 solver_b=False):
        import torch
        from . import mcts
        from .batch import BoardBatch
        self.pairs, self.sims, self.seed, self.opening_turns = int(pairs), sims, int(seed), int(opening_turns)
        self.sims_b = None if sims_b is None else int(sims_b)
        if self.sims_b is not None and (self.sims_b < 1 or sims < 1):
            raise ValueError("Arena: sims and sims_b must be at least 1")
        G = self.n = max(1, min(int(games_in_flight), 2 * self.pairs))
        self.env = BoardBatch(G, device)
        dev = self.device = self.env.device
        self.L = self.env._L
        self._ids = game_ids_of_pairs(pair_ids if pair_ids is not None else range(self.pairs))
        first = [next(self._ids, -1) for _ in range(G)]
        self._slot_game = list(first)
        self.game_id = torch.tensor(first, dtype=torch.int64, device=dev)
        self.active = torch.zeros((G,), dtype=torch.int8, device=dev)
        self.a_white = torch.zeros((G,), dtype=torch.int8, device=dev)
        self.pair_id = torch.zeros((G,), dtype=torch.int64, device=dev)
        rounds = sims if self.sims_b is None else max(sims, self.sims_b)
        self.search = mcts.ArenaSearch(G, rounds, evaluator_a, evaluator_b, self.a_white, dev.index, slots, seed,
                                       noise_eps=noise_eps, gumbel_a=gumbel_a, gumbel_b=gumbel_b,
                                       gumbel_interior_a=gumbel_interior_a, gumbel_interior_b=gumbel_interior_b,
                                       solver_a=solver_a, solver_b=solver_b, **(search_options or {}))
        self.budget = torch.zeros((G,), dtype=torch.int32, device=dev) if self.sims_b is not None else None
        self._assign()
        self.result_codes = torch.zeros((G,), dtype=torch.int8, device=dev)
        self.tally = torch.zeros((8,), dtype=torch.int32, device=dev)
        self.keep_moves = bool(keep_moves)
        self.moves = torch.full((G, MAX_MOVES), -3, dtype=torch.int16, device=dev) if keep_moves else None
        self._rows = torch.arange(G, device=dev)
        self.games, self.results = {}, {}
        self.plies = self.searches = 0

    def _assign(self):
        """Colour, pair and search keys of every slot from its game id (-1 = idle)."""
        import torch
        gid = self.game_id
        self.active.copy_(gid >= 0)
        self.a_white.copy_((gid >= 0) & (gid % 2 == 0))
        self.pair_id.copy_(torch.clamp(gid, min=0) // 2)
        self.search.set_game_ids(torch.clamp(gid, min=0))

    def running(self):
        """Number of slots that still hold a game."""
        return sum(1 for g in self._slot_game if g >= 0)

    def _retire_finished(self, boards):
        """Score the finished games; their slots take the next game ids.  -> number of games retired."""
        import torch
        from ._lib import check
        over, winner = self.env.terminal()
        check(self.L.hive_arena_score_launch(_p(boards), _p(over), _p(winner), _p(self.active), _p(self.a_white), self.n,
                                             MAX_GAME_LENGTH, _p(self.result_codes), _p(self.tally), stream_ptr(self.device)))
        codes = self.result_codes.cpu().numpy()
        slots = [int(s) for s in codes.nonzero()[0]]
        if not slots:
            return 0
        idx = torch.tensor(slots, dtype=torch.int64, device=self.device)
        if self.keep_moves:
            turns = boards[idx, 33].cpu().tolist()
            rows = self.moves[idx].cpu().tolist()
            self.moves[idx] = -3
        for k, s in enumerate(slots):
            gid, code = self._slot_game[s], int(codes[s])
            self.results[gid] = code
            if self.keep_moves:
                self.games[gid] = (code, rows[k][:max(0, min(turns[k] - 1, MAX_MOVES))])
            self._slot_game[s] = next(self._ids, -1)
        self.game_id[idx] = torch.tensor([self._slot_game[s] for s in slots], dtype=torch.int64, device=self.device)
        self._assign()
        self.env.reset(idx.to(torch.int32))
        return len(slots)

    def play_ply(self, forced=None):
        """One move for every running game.  Returns the number of games that finished before this move.
        forced: optional int32[games_in_flight]; entries >= -1 replace the move of that slot (-2 = keep the engine's)."""
        import torch
        from ._lib import check
        from .mcts import _override
        boards, hist = self.env.export_state()
        nd = self._retire_finished(boards)
        if nd:
            boards, hist = self.env.export_state()
        if not self.running():
            return nd
        _, count, lst = self.env.legal(want_list=True)
        turn = boards[:, 33]
        searched = ((self.active != 0) & (turn > self.opening_turns)).to(torch.int8)
        if bool(searched.any().item()):
            if self.budget is not None:
                check(self.L.hive_arena_budget_launch(_p(boards), _p(self.a_white), self.n, self.sims, self.sims_b,
                                                      _p(self.budget), stream_ptr(self.device)))
            action, _, _ = self.search.search(boards, hist, active=searched, selfplay=False,      # argmax of the visits
                                              budgets=self.budget)
            self.searches += 1
        else:
            action = self.search.action.fill_(-2)
        check(self.L.hive_arena_opening_launch(_p(boards), _p(count), _p(lst), _p(self.pair_id), _p(self.active), self.n,
                                               ctypes.c_uint64(self.seed & (2 ** 64 - 1)), self.opening_turns, _p(action),
                                               stream_ptr(self.device)))
        action = _override(action, forced)
        if self.keep_moves:
            col = torch.clamp(turn.long() - 1, 0, MAX_MOVES - 1).view(-1, 1)
            old = self.moves.gather(1, col)
            self.moves.scatter_(1, col, torch.where((action != -2).view(-1, 1), action.to(torch.int16).view(-1, 1), old))
        # the env re-derives the legal sets and refuses anything outside them: illegal_count() must stay 0
        self.env.step(action, sync=False)
        self.plies += 1
        return nd

    def run(self, max_plies=None):
        """Play every pair to the end -> ArenaResult."""
        limit = max_plies if max_plies is not None else (2 * self.pairs // self.n + 2) * (MAX_GAME_LENGTH + 1)
        while self.running():
            if self.plies >= limit:
                raise RuntimeError(f"Arena.run: {self.running()} games still running after {self.plies} plies")
            self.play_ply()
        return self.result()

    def result(self):
        """The match so far (the device tally is read here, once)."""
        return ArenaResult(self.tally.cpu().tolist(), pair_scores(self.results))

    def rows_evaluated(self):
        return self.search.rows_evaluated()

    def illegal_count(self):
        return self.env.illegal_count()

    def close(self):
        self.search.close()
        self.env.close()
