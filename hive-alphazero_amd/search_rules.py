"""The rules of the search stated in numpy: what the kernels behind include/hive_search.h draw, schedule and choose, as pure
functions a test or the sequential player (solo_play.py) can call without a GPU.  mcts.py re-exports every name.

This module imports neither torch nor the native library.
"""
import numpy as np

__all__ = ["PUCT", "UCT", "LEAF_KINDS", "BUDGET_STREAM", "GUMBEL_STREAM", "GUMBEL_DEFAULTS", "rng_word", "full_threshold",
           "playout_cap_draw", "rolling_clock_step", "rolling_quantum", "rolling_options", "gumbel_considered_visits",
           "gumbel_draw", "gumbel_improved_policy", "gumbel_options", "gumbel_interior_options", "gumbel_interior_choice"]

PUCT, UCT = 0, 1           # HiveSearchMode (include/hive_search.h)
LEAF_KINDS = ("unused", "root_evaluated", "expanded_evaluated", "known_finished_game", "collision", "length_cap",
              "new_finished_or_capped", "already_created_in_flight")


# ---- csrc/hive_rng.hpp: the counter-based generator, keyed (seed, a, b, c)
_M64 = (1 << 64) - 1


def _splitmix(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _u64(x):
    """x mod 2^64 as uint64: a Python int of any size or sign, or an integer array (int64 wraps, as the device's cast does)."""
    return np.uint64(x & _M64) if isinstance(x, int) else np.asarray(x).astype(np.uint64)


def rng_word(seed, a, b, c):
    """uint64 array: the first 64-bit output of csrc/hive_rng.hpp's generator Rng(seed, a, b, c) -- the word its first
    uniform() is made of -- for keys that broadcast against each other (Python ints or integer arrays, taken mod 2^64)."""
    with np.errstate(over="ignore"):
        inner = _splitmix(_u64(b) * np.uint64(0x9E3779B1) + _u64(c))
        s = _splitmix(_u64(seed) ^ _splitmix(_u64(a) * np.uint64(0x100000001B3) + inner))
        return np.asarray(_splitmix(s))


BUDGET_STREAM = 0x8CB92BA72F3D8DD7      # stream constant of hive_search_draw_budgets (include/hive_search.h)


def full_threshold(p_full):
    """floor(p_full * 2^32) saturated to 32 bits: what hive_search_draw_budgets compares the draw with (0xFFFFFFFF = always)."""
    if not 0.0 <= p_full <= 1.0:
        raise ValueError("p_full must lie in [0, 1]")
    return min(int(p_full * 4294967296.0), 0xFFFFFFFF)


def playout_cap_draw(seed, game_ids, turns, p_full):
    """bool[n]: is the ply of game game_ids[i] at root turn turns[i] searched in full?  The numpy restatement of
    hive_search_draw_budgets (no GPU): x = the first output of csrc/hive_rng.hpp's generator keyed by (seed ^ BUDGET_STREAM,
    game id, turn, 0); full iff (x >> 32) < floor(p_full * 2^32), and always at p_full = 1 (the saturated threshold)."""
    thr = full_threshold(p_full)
    if thr == 0xFFFFFFFF:
        return np.ones(len(game_ids), dtype=bool)
    x = rng_word(int(seed) ^ BUDGET_STREAM, np.asarray(game_ids, dtype=np.int64), np.asarray(turns, dtype=np.int64), 0)
    return (x >> np.uint64(32)) < np.uint64(thr)


def rolling_clock_step(clock, budget, active, slots):
    """One round of a rolling search in numpy (no GPU): the rule of search_select_kernel's per-game clocks and of
    hive_search_round_end.  clock / budget int[n], active bool-like[n] -> (takes_part bool[n, slots], clock after the round
    int64[n], done bool[n]).  An active game at clock c with budget b runs slot sl iff c + sl < b and (c > 0 or sl == 0) -- the
    root-opening simulation runs alone -- as simulation number c + sl; the round moves its clock by 1 from 0, else by
    min(slots, b - c); done = active and clock >= budget.  Iterated from 0 this lays a game's simulations out as
    TreeSearch.run_simulations does for sims = b: 0 alone, then `slots` per round."""
    c = np.asarray(clock, dtype=np.int64)
    b = np.asarray(budget, dtype=np.int64)
    on = np.asarray(active) != 0
    sl = np.arange(int(slots), dtype=np.int64)[None, :]
    part = on[:, None] & (c[:, None] + sl < b[:, None]) & ((c[:, None] > 0) | (sl == 0))
    step = np.where(c == 0, 1, np.minimum(int(slots), b - c))
    after = np.where(on & (c < b), c + step, c)
    return part, after, on & (after >= b)


def rolling_quantum(sims, slots):
    """Rounds a rolling search of `sims` simulations takes: the opening one alone, then `slots` per round."""
    return 1 + -(-(int(sims) - 1) // int(slots))


def rolling_options(rolling, search_options, sims, slots, playout_cap=None):
    """SelfPlay's `rolling` argument checked and completed (no GPU): None for lock step, else {"quantum": rounds per
    turn-over}.  rolling = None / False, True, or {"quantum": q}; the default quantum is the rounds of the shorter search,
    rolling_quantum(min(full, fast) with a cap else sims, slots).  search_options with keep_tree are refused with rolling:
    hive_search_advance_roots moves every tree at once."""
    if not rolling:
        return None
    opt = {} if rolling is True else dict(rolling)
    if set(opt) - {"quantum"}:
        raise ValueError("rolling takes True or {'quantum': rounds per turn-over}")
    if (search_options or {}).get("keep_tree"):
        raise ValueError("SelfPlay: rolling cannot keep trees (hive_search_advance_roots moves every tree at once)")
    shortest = min(playout_cap["full"], playout_cap["fast"]) if playout_cap else sims
    q = int(opt.get("quantum") or rolling_quantum(shortest, slots))
    if q < 1:
        raise ValueError("rolling: quantum must be at least 1")
    return {"quantum": q}


# ---- Gumbel root with sequential halving (include/hive_search.h, hive_search_set_gumbel): the numpy statements, no GPU
GUMBEL_STREAM = 0x6A09E667F3BCC909      # stream constant of the per-edge Gumbel draws
GUMBEL_DEFAULTS = {"m": 16, "c_visit": 50.0, "c_scale": 1.0}      # c_visit / c_scale: the paper's values, not tuned for this game


def gumbel_considered_visits(m, n):
    """int32[n]: the sequential-halving sequence of considered visits for m considered actions and n simulations (Danihelka
    et al. 2022, as the published mctx code lays it out).  m <= 1: 0 .. n-1.  Else with L = ceil(log2 m) and k = m: emit
    max(1, n // (L k)) times the visit counts of the first k slots, incrementing them after each emission, then
    k = max(2, k // 2), until n entries exist.  Simulation s >= 1 of a search goes to an edge that holds entry s - 1 visits."""
    m, n = int(m), max(int(n), 0)
    if m <= 1:
        return np.arange(n, dtype=np.int32)
    log2m = (m - 1).bit_length()
    seq, visits, k = [], [0] * m, m
    while len(seq) < n:
        for _ in range(max(1, n // (log2m * k))):
            seq.extend(visits[:k])
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return np.asarray(seq[:n], dtype=np.int32)


def gumbel_draw(seed, game_id, turn, ne, quiet=False):
    """float64[ne]: g_e = -log(-log(u_e)) of the root of game `game_id` at root turn `turn`; u_e (float32, computed exactly as
    the device does, like playout_cap_draw's word) is the first uniform of csrc/hive_rng.hpp's generator keyed
    (seed ^ GUMBEL_STREAM, game id, turn << 40, edge e) -- the noise key at simulation 0, slot 0.  quiet: zeros."""
    ne = int(ne)
    if quiet:
        return np.zeros(ne, dtype=np.float64)
    s = rng_word(int(seed) ^ GUMBEL_STREAM, int(game_id), int(turn) << 40, np.arange(ne, dtype=np.uint64))
    with np.errstate(divide="ignore"):
        u = ((s >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
        return -np.log(-np.log(u.astype(np.float64)))


def gumbel_improved_policy(p, n, w, v_root, c_visit=GUMBEL_DEFAULTS["c_visit"], c_scale=GUMBEL_DEFAULTS["c_scale"]):
    """(logit + sigma(completed q), improved policy) float64[ne] of a root with priors p, visits n, value sums w and the
    network value v_root: the rule of include/hive_search.h in float64.  The score of an edge is its g plus the first array;
    the improved policy is the softmax of the first array."""
    p = np.asarray(p, dtype=np.float64)
    n = np.asarray(n, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    logit = np.log(np.maximum(p, 1e-30))
    seen = n > 0
    q = np.where(seen, w / np.maximum(n, 1), 0.0)
    total, prior_seen = int(n.sum()), float(p[seen].sum())
    v_mix = float(v_root)
    if total > 0 and prior_seen > 0.0:
        v_mix = (float(v_root) + total * float((p[seen] * q[seen]).sum()) / prior_seen) / (1.0 + total)
    qhat = np.where(seen, q, v_mix)
    lo, hi = float(qhat.min()), float(qhat.max())
    sigma = (float(c_visit) + int(n.max())) * float(c_scale) * ((qhat - lo) / max(hi - lo, 1e-8))
    score = logit + sigma
    z = np.exp(score - score.max())
    return score, z / z.sum()


def gumbel_options(gumbel, slots=1, mode=PUCT, keep_tree=False):
    """TreeSearch's `gumbel` argument checked and completed (no GPU): None for off, else {"m", "c_visit", "c_scale"}.
    gumbel = None / False, True, or a dict with any of those keys (GUMBEL_DEFAULTS fill the rest).  Refused, as
    hive_search_set_gumbel refuses them: slots > 1 (visits in flight would desynchronise the halving schedule), UCT mode,
    and kept trees (a carried root has no network value of its own and no fresh schedule)."""
    if not gumbel:
        return None
    opt = {} if gumbel is True else dict(gumbel)
    if set(opt) - set(GUMBEL_DEFAULTS):
        raise ValueError("gumbel takes True or a dict with m, c_visit, c_scale")
    opt = {"m": int(opt.get("m", GUMBEL_DEFAULTS["m"])), "c_visit": float(opt.get("c_visit", GUMBEL_DEFAULTS["c_visit"])),
           "c_scale": float(opt.get("c_scale", GUMBEL_DEFAULTS["c_scale"]))}
    if opt["m"] < 1 or not opt["c_visit"] >= 0.0 or not opt["c_scale"] > 0.0:
        raise ValueError("gumbel: m must be at least 1, c_visit >= 0 and c_scale > 0")
    if int(slots) > 1:
        raise ValueError("gumbel: one slot only (visits in flight would desynchronise the sequential-halving schedule)")
    if mode == UCT:
        raise ValueError("gumbel: the Gumbel root has no UCT form (PUCT mode only)")
    if keep_tree:
        raise ValueError("gumbel: not with keep_tree (a carried root has no network value and no fresh schedule)")
    return opt


def gumbel_interior_options(gumbel_interior, gumbel):
    """TreeSearch's `gumbel_interior` argument checked (no GPU): True iff the Gumbel rule also selects below the root.  It is an
    option of the Gumbel root, not a search of its own: without `gumbel` it is refused."""
    if gumbel_interior and not gumbel:
        raise ValueError("gumbel_interior: needs the Gumbel root (gumbel=True or its option dict)")
    return bool(gumbel_interior)


def gumbel_interior_choice(p, n, w, v_node, c_visit=GUMBEL_DEFAULTS["c_visit"], c_scale=GUMBEL_DEFAULTS["c_scale"]):
    """(edge, score float64[ne]) of the Gumbel rule below the root at a node with priors p, visits n, value sums w and the value
    v_node its position was predicted with (include/hive_search.h, hive_search_set_gumbel_interior), in float64:
    score = improved policy - n / (1 + sum n); the edge is the first maximum.  A single edge is taken as it is."""
    n = np.asarray(n, dtype=np.int64)
    if n.size == 1:
        return 0, np.zeros(1)
    _, improved = gumbel_improved_policy(p, n, w, v_node, c_visit, c_scale)
    score = improved - n / (1.0 + float(n.sum()))
    return int(np.argmax(score)), score


# ---- Proven wins and losses below the root (include/hive_search.h, hive_search_set_solver): the numpy statements, no GPU
# (imported by name: mcts.py re-exports them next to the names of __all__)
def solver_edge_status(child_status):
    """The status of an edge whose child has status `child_status` (int or int array), from the mover at the edge's parent:
    -sign(c) * (|c| + 1), and 0 for an unknown child."""
    c = np.asarray(child_status, dtype=np.int64)
    out = -np.sign(c) * (np.abs(c) + 1)
    return int(out) if out.ndim == 0 else out


def solver_node_status(edge_status):
    """The status of a node from the statuses of ALL its edges: the smallest positive one if any edge wins (the fastest win),
    else -max|e| if every edge loses (the longest resistance), else 0.  An edge that is not expanded holds 0 and blocks a
    loss proof; the pass edge is an edge like any other."""
    e = np.asarray(edge_status, dtype=np.int64).reshape(-1)
    if (e > 0).any():
        return int(e[e > 0].min())
    if e.size and (e < 0).all():
        return -int(np.abs(e).max())
    return 0


def solver_holds(status, turn, cap):
    """Does a status (node or edge; int or int array) hold on a path whose current turn is `turn`?  Iff it is not 0 and the
    finished position lies within the length cap: turn + |status| - 1 <= cap."""
    x = np.asarray(status, dtype=np.int64)
    out = (x != 0) & (int(turn) + np.abs(x) - 1 <= int(cap))
    return bool(out) if out.ndim == 0 else out


def solver_answer(edge_status, n, turn, cap):
    """(edge, allowed bool[ne]): the answer at a root at turn `turn` whose edges hold `edge_status` and the visits n.
    edge >= 0: the move comes from a proof -- the root's status (solver_node_status of its edges) holds and is positive:
    the smallest positive status that holds; or negative: the largest |e|; ties to more visits, then to the lower edge.
    edge = -1: no proof; the caller's own choice runs over the edges with allowed[e] -- every edge but those whose status
    holds and is negative, unless every edge is such."""
    e = np.asarray(edge_status, dtype=np.int64).reshape(-1)
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    holds = solver_holds(e, turn, cap) if e.size else np.zeros(0, dtype=bool)
    banned = holds & (e < 0)
    allowed = ~banned if not banned.all() else np.ones(e.size, dtype=bool)
    root = solver_node_status(e)
    if not solver_holds(root, turn, cap):
        return -1, allowed
    cand = np.flatnonzero(holds & ((e > 0) == (root > 0)))
    speed = -e[cand] if root > 0 else np.abs(e[cand])      # larger is better: the fastest win, the longest resistance
    order = sorted(zip((-speed).tolist(), (-n[cand]).tolist(), cand.tolist()))
    return int(order[0][2]), allowed


def solver_options(solver, mode=PUCT, gumbel=None):
    """TreeSearch's `solver` argument checked (no GPU): True iff proven wins and losses are on.  Refused, as
    hive_search_set_solver refuses them: UCT mode, and together with the Gumbel root (its halving schedule counts root visits,
    and a proven root ends descents at depth 0)."""
    if not solver:
        return False
    if solver is not True and solver != 1:
        raise ValueError("solver takes True or False")
    if mode == UCT:
        raise ValueError("solver: proven results have no UCT form (PUCT mode only)")
    if gumbel:
        raise ValueError("solver: not with the Gumbel root (its halving schedule counts root visits)")
    return True
