"""HivePlayer: the reference-sequential search behind the drop-in API of woker/solo_play.py.

Same constructor, attributes and `action(env) -> (move, [policy list, visit total])` contract as the
reference's HivePlayer (woker/solo_play.py:69-384), and the same search process: a transposition
table keyed by env.state_key, one evaluator call per simulation, virtual loss, fresh Dirichlet
noise on the root priors at every simulation, visit-count policy with the "all W negative ->
priors" fallback, argmax temperature.  With SEARCH_THREADS = 1 and a seeded numpy it reproduces the
reference's visit counts, W sums, priors and chosen move bit for bit (tests/test_mcts_golden.py).

The implementation is this repo's own: each table entry keeps its edges in flat numpy arrays
(struct-of-arrays, like the GPU search in csrc/hive_search.hip), a simulation is an explicit
descent/backup over a path stack instead of a recursion, and PUCT is one vectorised expression.
Arithmetic is arranged so that every floating-point operation happens in the reference's order and
dtype (float32 priors, float64 scores), and the numpy RNG is consumed by the same two calls.

It is env-agnostic (anything with the GamePlay API) and talks to the evaluator through the pipe
protocol (send(planes) / recv() -> (p[1584], v)).  The throughput path is hive_alphazero_amd.mcts.
"""
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from copy import deepcopy
from threading import Lock

import numpy as np

from . import config
from .config import ACTION_SPACE, MAX_GAME_LENGTH, PIECE_BLACK, PIECE_WHITE
from .search_rules import (GUMBEL_DEFAULTS, gumbel_considered_visits, gumbel_improved_policy, gumbel_interior_choice,
                           solver_answer, solver_edge_status, solver_holds, solver_node_status)

# woker/solo_play.py:23-30 (module-level knobs, same names so callers can override them the same way)
simulation_num_per_move = 100
tau_decay_rate = 0.01
c_puct = 0.7
dirichlet_alpha = 0.3
noise_eps = 0.25
virtual_loss = 1
SEARCH_THREADS = config.SEARCH_THREADS

_DRAW = 5          # sentinel a drawn / length-capped line returns (solo_play.py:180-183)


class _Entry:
    """One position of the transposition table: raw network priors until its first selection, then
    per-edge arrays in legal-move order."""
    __slots__ = ("raw_p", "moves", "n", "w", "p", "sum_n", "v", "status", "es")

    def __init__(self, raw_p, v=0.0):
        self.raw_p = raw_p
        self.v = v                     # the value this position was predicted with (the Gumbel rule below the root reads it)
        self.moves = None
        self.n = self.w = self.p = None
        self.sum_n = 0
        self.status = 0                # proven result from the side to move here (HivePlayer.solver), 0 = unknown
        self.es = None                 # per-edge statuses from the mover's side, with the other edge arrays

    def open_edges(self, legal):
        """First selection at this position: priors of the legal moves, renormalised with the reference's
        running float32 total that starts at 1e-8 (solo_play.py:304-313)."""
        prior = np.asarray(self.raw_p)[legal]
        running = np.cumsum(np.concatenate((np.asarray([1e-8], dtype=prior.dtype), prior)), dtype=prior.dtype)
        self.moves = list(legal)
        self.p = prior / running[-1]
        self.n = np.zeros(len(legal), dtype=np.int64)
        self.w = np.zeros(len(legal), dtype=np.float64)
        self.es = np.zeros(len(legal), dtype=np.int64)
        self.raw_p = None

    def q(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.n > 0, self.w / self.n, 0.0)


class _EdgeView:
    """Read-only per-edge record (n, w, q, p) for callers that inspect `player.tree[key].a`."""
    __slots__ = ("n", "w", "q", "p")

    def __init__(self, n, w, p):
        self.n, self.w, self.p = int(n), float(w), p
        self.q = self.w / self.n if self.n else 0


class _EntryView:
    def __init__(self, entry):
        self.sum_n = entry.sum_n if entry is not None else 0
        self.a = {}
        if entry is not None and entry.moves is not None:
            for i, m in enumerate(entry.moves):
                self.a[m] = _EdgeView(entry.n[i], entry.w[i], entry.p[i])


class _TreeView:
    """`player.tree[state_key]` -> object with `.a` (move -> edge record) and `.sum_n`, `len(player.tree)`."""

    def __init__(self, table):
        self._t = table

    def __getitem__(self, key):
        return _EntryView(self._t.get(key))

    def __contains__(self, key):
        return key in self._t

    def __len__(self):
        return len(self._t)


def _terminal_value(env):
    """Value of a finished position from the side to move, or the draw sentinel (solo_play.py:169-183)."""
    if env.game_is_over():
        winner = env.state.winner
        mover_is_white = env.state.player() == 0
        if winner == PIECE_WHITE:
            return 1 if mover_is_white else -1
        if winner == PIECE_BLACK:
            return -1 if mover_is_white else 1
        return _DRAW
    if env.state.turn >= MAX_GAME_LENGTH:
        return _DRAW
    return None


class HivePlayer:
    def __init__(self, pipes=None, reward=False):
        self.moves = []
        self.pipe_pool = pipes
        self.none_queue = True
        self.net = None
        self.simulation_num_per_move = simulation_num_per_move
        self.reward = reward
        self.main_key_state = None
        self.max_depth = None
        self._table = {}
        self._locks = defaultdict(Lock)
        self.solver_stats = [0, 0, 0, 0]

    # ------------------------------------------------------------------ reference surface
    @property
    def tree(self):
        return _TreeView(self._table)

    def reset(self):
        self._table = {}

    # True: action() keeps the part of the table that lies under env's position instead of emptying it (the sequential
    # statement of hive_search_advance_roots, include/hive_search.h).  False: the reference, solo_play.py:103-112.
    keep_tree = False

    def keep_reachable(self, env):
        """Prune the table to the entries reachable from env's position through visited edges (n > 0), walking copies of
        env: a finished or length-capped position ends a line, a position only an unvisited edge leads to is forgotten
        (and evaluated again when it is reached)."""
        kept = {}
        todo = [deepcopy(env)]
        while todo:
            at = todo.pop()
            if _terminal_value(at) is not None:
                continue
            key = at.state_key
            entry = self._table.get(key)
            if entry is None or key in kept:
                continue
            kept[key] = entry
            if entry.moves is None:
                continue
            for edge, move in enumerate(entry.moves):
                if entry.n[edge] > 0:
                    nxt = deepcopy(at)
                    nxt.move(move)
                    todo.append(nxt)
        self._table = kept

    # None: the reference.  A dict switches the root to the Gumbel root with sequential halving, the sequential statement of
    # hive_search_set_gumbel (the rule: include/hive_search.h): {"m": 16, "c_visit": 50.0, "c_scale": 1.0, "g": ...}.  "g" is
    # the caller's: an array of one Gumbel draw per root edge (ascending action id), a callable (root turn, edges) -> such an
    # array (e.g. search_rules.gumbel_draw with a seed and game id bound), or None / absent for zeros (a quiet game).  Simulation
    # s >= 1 takes the best-scoring root edge among those holding the visit count the schedule asks for, action() plays the
    # best-scoring edge among the most visited and calc_policy() returns the improved policy.  Below the root: PUCT, no noise.
    # SEARCH_THREADS = 1 only; not with keep_tree.  After action(): gumbel_fallbacks = selections that found no edge at the
    # scheduled count, gumbel_min_gap = the smallest strictly positive gap between the two best scores over those selections
    # and the final choice (inf if none).
    # "interior": True -- the Gumbel rule below the root as well (hive_search_set_gumbel_interior): at depth >= 1 the edge is
    # the first maximum of improved policy - n / (1 + sum n), the improved policy taken with the value the entry's position
    # was predicted with (search_rules.gumbel_interior_choice); no noise, no c_puct.  gumbel_min_gap then covers those selections
    # too, and gumbel_interior_min_gap holds theirs alone.
    gumbel = None

    # True: proven wins and losses below the root, the sequential statement of hive_search_set_solver (the rule:
    # include/hive_search.h).  Every table entry keeps a status and per-edge statuses, updated along the path after the
    # reference's backup; a descent ends at an entry whose status holds, moves proven to lose are left out of PUCT and of the
    # answer, and a proven root answers from the proof.  The policy and the visit total are the reference's.  After action():
    # solver_stats = [descents ended at a proven entry, entries that became proven wins, proven losses, answers from a proof]
    # since the player was made.  Not with `gumbel`.  False: the reference.
    solver = False

    def action(self, env, non_queue=True):
        if self.keep_tree:
            self.keep_reachable(env)
        else:
            self.reset()
        self.max_depth = env.state.turn
        self.main_key_state = env.state_key
        if self.solver:
            if self.gumbel is not None or (self.none_queue and SEARCH_THREADS > 1):
                raise ValueError("HivePlayer.solver: sequential PUCT search only, not with gumbel")
        if self.gumbel is not None:
            if self.keep_tree or (self.none_queue and SEARCH_THREADS > 1):
                raise ValueError("HivePlayer.gumbel: sequential search without kept trees only")
            self._sim, self._root_v, self._root_g = 0, 0.0, None
            self.gumbel_fallbacks, self.gumbel_min_gap = 0, float("inf")
            self.gumbel_interior_min_gap = float("inf")
        self.search_moves(env)
        policy, visits = self.calc_policy(env)
        if self.gumbel is not None:
            return self._gumbel_move(env), [list(policy), visits]
        choice = policy
        if self.solver:
            entry = self._table[env.state_key]
            if entry.moves is not None:
                edge, allowed = solver_answer(entry.es, entry.n, env.state.turn, MAX_GAME_LENGTH)
                if edge >= 0:
                    self.solver_stats[3] += 1
                    return int(entry.moves[edge]), [list(policy), visits]
                if not allowed.all():                        # the moves proven to lose leave the choice, not the policy
                    choice = np.array(policy, dtype=np.float64)
                    choice[np.asarray(entry.moves)[~allowed]] = -1.0
        probs = self.apply_temperature(choice, int(env.state.turn + 1) / 2)
        move = int(np.random.choice(range(ACTION_SPACE), p=probs))
        return move, [list(policy), visits]

    def search_moves(self, env):
        if self.none_queue and SEARCH_THREADS > 1:
            with ThreadPoolExecutor(max_workers=SEARCH_THREADS) as pool:
                jobs = [pool.submit(self.search_my_move, deepcopy(env), True)
                        for _ in range(self.simulation_num_per_move)]
            values = [j.result() for j in jobs]
        else:
            values = [self.search_my_move(deepcopy(env), True) for _ in range(self.simulation_num_per_move)]
        return np.max(values), values[0]

    def search_my_move(self, env, is_root_node=False):
        """One simulation from `env` (consumed): returns the value seen from its side to move."""
        path = []                      # (entry, edge index) from the root down
        outcome = None
        depth = 0
        proven = 0                     # solver: the status of the position where the path ends
        if self.gumbel is not None and is_root_node:
            self._cur_sim, self._sim = self._sim, self._sim + 1       # simulations of a search are numbered 0, 1, ...
        while True:
            outcome = _terminal_value(env)
            if outcome is not None:
                if self.solver and outcome != _DRAW and env.game_is_over():
                    proven = int(outcome)                    # only a finished game with a winner proves anything
                break
            key = env.state_key
            with self._locks[key]:
                entry = self._table.get(key)
                if entry is None:
                    leaf_p, leaf_v = self._evaluate(env)
                    self._table[key] = _Entry(leaf_p, float(np.asarray(leaf_v).reshape(-1)[0]))
                    outcome = leaf_v
                    if self.gumbel is not None and is_root_node and depth == 0:
                        self._root_v = float(np.asarray(leaf_v).reshape(-1)[0])      # completes the unvisited root edges
                    break
                if self.solver and solver_holds(entry.status, env.state.turn, MAX_GAME_LENGTH):
                    proven = entry.status                    # a proven position ends the descent like a finished game
                    outcome = 1 if proven > 0 else -1
                    self.solver_stats[0] += 1
                    break
                edge, move = self._select(entry, env, is_root_node and depth == 0)
                entry.sum_n += virtual_loss                 # virtual loss (solo_play.py:205-208)
                entry.n[edge] += virtual_loss
                entry.w[edge] -= virtual_loss
            path.append((key, entry, edge))
            env.move(move)
            depth += 1
            if env.state.turn > self.max_depth:
                self.max_depth = env.state.turn
        # backup, deepest edge first; a drawn line scores -1 at every ply and stays a draw (solo_play.py:217-247)
        value = outcome
        for key, entry, edge in reversed(path):
            drawn = value == _DRAW
            seen = -1 if drawn else -value
            with self._locks[key]:
                entry.sum_n += -virtual_loss + 1
                entry.n[edge] += -virtual_loss + 1
                entry.w[edge] += virtual_loss + seen
            value = _DRAW if drawn else seen
        if proven:
            # proven results travel up this path, deepest edge first: the edge takes the child's status seen from the mover,
            # the entry is decided by all of its edges
            result = value
            for key, entry, edge in reversed(path):
                if abs(proven) >= 127:
                    break
                with self._locks[key]:
                    entry.es[edge] = solver_edge_status(proven)
                    status = solver_node_status(entry.es)
                    if entry.status == 0 and status != 0:
                        self.solver_stats[1 if status > 0 else 2] += 1
                    entry.status = proven = status
                if proven == 0:
                    break
            return result
        return value

    def expand_and_evaluate(self, env):
        return self.predict(env.encode_board())

    def expand_and_evaluate_with_net(self, env):
        import torch
        planes = np.ascontiguousarray(env.encode_board().transpose(2, 0, 1))
        dev = next(self.net.parameters()).device
        with torch.no_grad():
            p, v = self.net(torch.from_numpy(planes).float().to(dev).unsqueeze(0))
        return p.cpu().numpy().reshape(-1), v.cpu().numpy().reshape(-1)

    def _evaluate(self, env):
        return self.expand_and_evaluate(env) if self.none_queue else self.expand_and_evaluate_with_net(env)

    def predict(self, board_state):
        pipe = self.pipe_pool.pop()
        pipe.send(board_state)
        answer = pipe.recv()
        self.pipe_pool.append(pipe)
        return answer

    def select_action_q_and_u(self, env, is_root_node):
        """PUCT choice at env's position (solo_play.py:294-335); -1 when there is no legal move."""
        entry = self._table[env.state_key]
        return self._select(entry, env, is_root_node)[1]

    def _select(self, entry, env, at_root):
        legal = env.actions()
        if len(legal) == 0:
            if entry.moves is None:                          # the pass edge (solo_play.py:299-300)
                entry.moves, entry.raw_p = [-1], None
                entry.n, entry.w = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float64)
                entry.p = np.zeros(1, dtype=np.float64)
                entry.es = np.zeros(1, dtype=np.int64)
            return 0, -1
        if entry.moves is None:
            entry.open_edges(legal)
        if at_root and self.gumbel is not None:
            return self._gumbel_select(entry, env)
        if self.gumbel is not None and self.gumbel.get("interior"):
            return self._gumbel_interior_select(entry)
        prior = entry.p
        if at_root:
            noise = np.random.dirichlet([dirichlet_alpha] * len(entry.moves))
            prior = (1 - noise_eps) * prior + noise_eps * noise
        score = entry.q() + c_puct * prior * np.sqrt(entry.sum_n + 1) / (1 + entry.n)
        if self.solver:
            banned = solver_holds(entry.es, env.state.turn, MAX_GAME_LENGTH) & (entry.es < 0)
            if banned.any() and not banned.all():            # moves proven to lose are left out unless every move is one
                score = np.where(banned, -np.inf, score)
        edge = int(np.argmax(score))
        return edge, entry.moves[edge]

    # ------------------------------------------------------------------ Gumbel root (sequential statement)
    def _gumbel_scores(self, entry, env):
        """(g + logit + sigma, improved policy) over the root's edges."""
        opt = self.gumbel
        if self._root_g is None:
            g = opt.get("g")
            if callable(g):
                g = g(int(env.state.turn), len(entry.moves))
            self._root_g = np.zeros(len(entry.moves)) if g is None else np.asarray(g, dtype=np.float64)
            assert self._root_g.shape == (len(entry.moves),)
        base, improved = gumbel_improved_policy(entry.p, entry.n, entry.w, self._root_v,
                                                opt.get("c_visit", GUMBEL_DEFAULTS["c_visit"]),
                                                opt.get("c_scale", GUMBEL_DEFAULTS["c_scale"]))
        return self._root_g + base, improved

    def _gumbel_best(self, score, eligible):
        """First maximum of score over the eligible edges (ties to the lower edge); the top-two gap is recorded."""
        masked = np.where(eligible, score, -np.inf)
        edge = int(np.argmax(masked))
        rest = np.delete(masked, edge)
        if rest.size and np.isfinite(rest.max()) and masked[edge] - rest.max() > 0:
            self.gumbel_min_gap = min(self.gumbel_min_gap, float(masked[edge] - rest.max()))
        return edge

    def _gumbel_select(self, entry, env):
        score, _ = self._gumbel_scores(entry, env)
        m_eff = min(int(self.gumbel.get("m", GUMBEL_DEFAULTS["m"])), len(entry.moves))
        t = int(gumbel_considered_visits(m_eff, self.simulation_num_per_move - 1)[self._cur_sim - 1])
        eligible = entry.n == t
        if not eligible.any():                              # a root visit off the schedule (a line back into the root position)
            eligible = np.ones(len(entry.moves), dtype=bool)
            self.gumbel_fallbacks += 1
        edge = self._gumbel_best(score, eligible)
        return edge, entry.moves[edge]

    def _gumbel_interior_select(self, entry):
        """The Gumbel rule below the root: the edge whose visit share lags the improved policy most."""
        opt = self.gumbel
        edge, score = gumbel_interior_choice(entry.p, entry.n, entry.w, entry.v,
                                             opt.get("c_visit", GUMBEL_DEFAULTS["c_visit"]),
                                             opt.get("c_scale", GUMBEL_DEFAULTS["c_scale"]))
        rest = np.delete(score, edge)
        if rest.size and score[edge] - rest.max() > 0:
            gap = float(score[edge] - rest.max())
            self.gumbel_min_gap = min(self.gumbel_min_gap, gap)
            self.gumbel_interior_min_gap = min(self.gumbel_interior_min_gap, gap)
        return edge, entry.moves[edge]

    def _gumbel_move(self, env):
        entry = self._table[env.state_key]
        if entry.moves is None or entry.moves == [-1]:
            return -1
        score, _ = self._gumbel_scores(entry, env)
        return int(entry.moves[self._gumbel_best(score, entry.n == entry.n.max())])

    def apply_temperature(self, policy, turn):
        tau = np.power(tau_decay_rate, turn)
        if tau < 0.1:                                        # always true for turn >= 1: greedy
            greedy = np.zeros(ACTION_SPACE)
            greedy[np.argmax(policy)] = 1.0
            return greedy
        sharpened = np.power(policy, 1 / tau)
        return sharpened / np.sum(sharpened)

    def calc_policy(self, env):
        """Visit distribution at the root; the priors when every W is negative (solo_play.py:351-374)."""
        entry = self._table[env.state_key]
        if self.gumbel is not None:
            # the improved policy over the root's edges; the visit total is unchanged (the pass edge writes nothing)
            policy, total = np.zeros(ACTION_SPACE), 0
            if entry.moves is None and len(env.actions()) > 0:
                entry.open_edges(env.actions())            # a search of one simulation: the root was evaluated, never selected
            if entry.moves is not None and entry.moves != [-1]:
                policy[np.asarray(entry.moves)] = self._gumbel_scores(entry, env)[1]
                total = int(np.sum(entry.n))
            return policy, total
        visits = np.zeros(ACTION_SPACE)
        priors = np.zeros(ACTION_SPACE)
        if entry.moves is not None:
            for i, m in enumerate(entry.moves):
                visits[m] = entry.n[i]
                priors[m] = entry.p[i]
        total = np.sum(visits)
        policy = visits / np.sum(visits)
        if entry.moves is not None and np.max(entry.w) < 0:
            policy = priors
        return policy, total

    def finish_game(self, z):
        for move in self.moves:
            move += [z]
