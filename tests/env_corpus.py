"""Seeded oracle playouts that reach the rare corners of the rules engine, torus translation of positions, and coverage
counters over a list of positions.  TEST INFRASTRUCTURE, CPU-only: imported by tests, never by the product package.

Policies (each plays a uniform-random legal move with the probability in P_RANDOM, a forced pass as -1):
  uniform  every move uniform-random
  drift    the destination furthest along a direction drawn per game: the hive walks to the border of the 12x12 board and
           over it (the neighbour tables are a torus, the reference's straight-line test is not: DESIGN.md, Grasshopper)
  stack    a Beetle onto the highest stack it can reach
  crowd    a move that adds a neighbour to either queen
"""
from collections import namedtuple

import numpy as np

from oracle import oracle_py as O

POLICIES = ("uniform", "drift", "stack", "crowd")
P_RANDOM = {"uniform": 1.0, "drift": 0.30, "stack": 0.25, "crowd": 0.30}
DRIFT_DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
MAX_TURN = 55

Position = namedtuple("Position", "turn pos lvl mode legal over winner")

_NBR = None


def neighbours():
    """list of six neighbour cells per cell (the oracle's torus table)."""
    global _NBR
    if _NBR is None:
        _NBR = [set(row) for row in O.tables()[0].tolist()]
    return _NBR


def snapshot(g):
    pos, lvl = g.pieces()
    over, winner = g.game_is_over()
    return Position(int(g.turn), pos, np.where(pos == 255, 0, lvl).astype(np.uint8), int(g.nmt_mode), g.actions(), over, winner)


def drift_score(action, direction):
    """How far along `direction` the destination of `action` lies (board coordinates, no wrap)."""
    q, r = divmod(action // 11, 12)
    return direction[0] * q + direction[1] * r


def choose(policy, p, rng, direction=None):
    """The policy's move at Position p (-1 when nothing is legal).  Uses the position and its legal ids only."""
    acts = p.legal
    if not acts:
        return -1
    if rng.random() < P_RANDOM[policy]:
        return int(acts[rng.integers(len(acts))])
    own = 0 if p.turn % 2 == 1 else 11
    cand = []
    if policy == "drift":
        best = max(drift_score(a, direction) for a in acts)
        cand = [a for a in acts if drift_score(a, direction) == best]
    elif policy == "stack":
        height = {}
        for c, l in zip(p.pos.tolist(), p.lvl.tolist()):
            if c != 255:
                height[c] = max(height.get(c, 0), l + 1)
        onto = [a for a in acts if a % 11 in (1, 2) and a // 11 in height]
        if onto:
            top = max(height[a // 11] for a in onto)
            cand = [a for a in onto if height[a // 11] == top]
        else:
            cand = [a for a in acts if a % 11 in (1, 2)]
    elif policy == "crowd":
        nbr = neighbours()
        for q in (p.pos[0], p.pos[11]):
            if q == 255:
                continue
            near = nbr[int(q)]
            cand += [a for a in acts if a // 11 in near and int(p.pos[own + a % 11]) not in near]
    if cand:
        return int(cand[rng.integers(len(cand))])
    return int(acts[rng.integers(len(acts))])


def play_game(policy, rng):
    """One oracle game under `policy`: the list of its Positions (the last one is finished or at the turn cap)."""
    direction = DRIFT_DIRS[rng.integers(len(DRIFT_DIRS))] if policy == "drift" else None
    g = O.OracleGame()
    out = []
    while True:
        p = snapshot(g)
        out.append(p)
        if p.over or p.turn >= MAX_TURN:
            return out
        g.move(choose(policy, p, rng, direction))


def playout(policy, n_positions, seed):
    """At least n_positions Positions from whole seeded games under `policy`, truncated to n_positions."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_positions:
        out += play_game(policy, rng)
    return out[:n_positions]


def finished_with_previous(n_finished, seed):
    """(previous position, finished position) pairs from `crowd` games, n_finished of them, alternating winners as far
    as the games allow (both winners are always present)."""
    rng = np.random.default_rng(seed)
    by_winner = {1: [], 2: []}
    while min(len(v) for v in by_winner.values()) < n_finished // 2:
        game = play_game("crowd", rng)
        if game[-1].over and game[-1].winner in by_winner:
            by_winner[game[-1].winner].append((game[-2], game[-1]))
    return by_winner[1][:n_finished // 2] + by_winner[2][:n_finished - n_finished // 2]


# ---------------------------------------------------------------- translation

def translate(pos, dq, dr):
    """Cells (q, r) -> ((q + dq) mod 12, (r + dr) mod 12); 255 (in hand) stays.  Mode-0 positions only: modes 1 and 2
    name the start tile.  pos: uint8 array of any shape."""
    pos = np.asarray(pos, dtype=np.uint8)
    q, r = np.divmod(pos.astype(np.int32), 12)
    moved = ((q + dq) % 12) * 12 + (r + dr) % 12
    return np.where(pos == 255, 255, moved).astype(np.uint8)


OFFSETS = [(dq, dr) for dq in range(12) for dr in range(12)]


def translated_boards(positions):
    """All 144 translates of each mode-0 position, position-major: (turn[n*144], pos[n*144,22], lvl[n*144,22], mode)."""
    assert all(p.mode == 0 for p in positions)
    pos = np.stack([translate(p.pos, dq, dr) for p in positions for dq, dr in OFFSETS])
    lvl = np.repeat(np.stack([p.lvl for p in positions]), 144, axis=0)
    turn = np.repeat(np.array([p.turn for p in positions], dtype=np.uint8), 144)
    return turn, pos, lvl, np.zeros(len(turn), dtype=np.uint8)


def untranslate_masks(masks):
    """uint8[n*144, 1584] legal masks of translated_boards -> [n, 144, 144 cells, 11] with every mask moved back into
    the base position's frame, so that an equivariant rule gives 144 equal rows."""
    m = masks.reshape(-1, 12, 12, 12, 12, 11)                 # [n, dq, dr, q, r, slot]
    out = np.empty_like(m)
    for dq in range(12):
        for dr in range(12):
            out[:, dq, dr] = np.roll(m[:, dq, dr], (-dq, -dr), axis=(1, 2))
    return out.reshape(-1, 144, 144, 11)


def seam_rule(positions, stop_at=None):
    """Per mode-0 position: does it show the seam rule, i.e. is its own legal set not the most common one among its 144
    translates (moved back into its frame)?  With stop_at, counting ends once that many show it (the rest are False)."""
    shows = np.zeros(len(positions), dtype=bool)
    for lo in range(0, len(positions), 64):
        chunk = positions[lo:lo + 64]
        _, masks = O.batch_legal(*translated_boards(chunk))
        base = untranslate_masks(masks).reshape(len(chunk), 144, 1584)
        for i, rows in enumerate(base):
            keys = [r.tobytes() for r in np.packbits(rows, axis=1)]
            counts = {}
            for k in keys:
                counts[k] = counts.get(k, 0) + 1
            shows[lo + i] = counts[keys[0]] < max(counts.values())
        if stop_at is not None and shows.sum() >= stop_at:
            break
    return shows


# ---------------------------------------------------------------- coverage

def touches_seam(p):
    """Does a piece stand in row or column 0 or 11?"""
    q, r = np.divmod(p.pos[p.pos != 255], 12)
    return bool(np.any((q == 0) | (q == 11) | (r == 0) | (r == 11)))


def coverage(positions):
    """Counters over a list of Positions: per-cell occupancy (positions in which the cell holds a piece), histogram of the
    highest stack index per position, finished positions by winner (0 = draw), zero-legal positions, positions that touch
    row or column 0/11 among the mode-0 ones, and colours to move."""
    cells = np.zeros(144, dtype=np.int64)
    stack = np.zeros(8, dtype=np.int64)
    finished = {0: 0, 1: 0, 2: 0}
    zero_legal = mode0 = seam_touch = 0
    to_move = [0, 0]
    for p in positions:
        on = np.unique(p.pos[p.pos != 255])
        cells[on] += 1
        stack[int(p.lvl[p.pos != 255].max()) if len(on) else 0] += 1
        if p.over:
            finished[p.winner] += 1
        zero_legal += not p.legal
        to_move[(p.turn + 1) % 2] += 1
        if p.mode == 0:
            mode0 += 1
            seam_touch += touches_seam(p)
    return {"cells": cells, "stack": stack, "finished": finished, "zero_legal": int(zero_legal), "mode0": mode0,
            "seam_touch": seam_touch, "to_move": to_move}


def from_record(rec):
    """A golden-fixture ply (oracle/gen_golden.py snapshot) as a Position."""
    mode = 1 if rec["t"] == 1 else (2 if rec["t"] == 2 else 0)
    return Position(rec["t"], np.array(rec["pos"], dtype=np.uint8), np.array(rec["lvl"], dtype=np.uint8), mode,
                    rec["legal"], rec["over"], rec["win"])


# ---------------------------------------------------------------- the translated corpus of the GPU tests

def translated_corpus(n=256, seed=2024, pool=4000):
    """n mode-0 positions drawn evenly from the four policies.  From each policy's pool of `pool` positions: first zero-legal
    ones (at most an eighth of the policy's share), then ones with a stack index >= 3 (at most a third), then a seeded
    sample of the rest; so the rare states are in without being all there is."""
    share = n // len(POLICIES)
    out = []
    for k, policy in enumerate(POLICIES):
        cand = [p for p in playout(policy, pool, seed + k) if p.mode == 0 and not p.over]
        rng = np.random.default_rng(seed + 100 + k)
        order = rng.permutation(len(cand)).tolist()
        zero = [i for i in order if not cand[i].legal][:share // 8]
        tall = [i for i in order if cand[i].legal and cand[i].lvl.max() >= 3][:share // 3]
        rest = [i for i in order if i not in set(zero + tall)][:share - len(zero) - len(tall)]
        out += [cand[i] for i in zero + tall + rest]
    return out
