"""The slide step of the Ant flood and the Spider walk in its pull form (csrc/hive_bb.hpp: pull_step) against the push form
(slide_step) and against a cell-by-cell model of the gate rule: the algebra on a numpy model of the 12x12 hex torus (no
GPU), both device forms in both lane layouts through hive_debug_slide_step, and the legal-move launch against the CPU
oracle at the sizes where a wave is full, one short and one over."""
import ctypes

import numpy as np
import pytest

N = 12
# d0..d5 = R UR U L DL D as (row step, column step); the flanks of a step along d_i are c + d_(i-1) and c + d_(i+1)
DIRS = [(0, 1), (1, 1), (1, 0), (0, -1), (-1, -1), (-1, 0)]


# ------------------------------------------------------------------ the model: boards are bool[12][12] (row, column)
def up(x): return np.roll(x, 1, axis=0)          # row j -> j + 1
def down(x): return np.roll(x, -1, axis=0)
def right(x): return np.roll(x, 1, axis=1)       # column c -> c + 1
def left(x): return np.roll(x, -1, axis=1)


def views(occ):
    """S_i[c] = occ[c + d_i]"""
    return [np.roll(occ, (-dj, -dc), axis=(0, 1)) for dj, dc in DIRS]


def gates(occ):
    S = views(occ)
    cs = [S[(i - 1) % 6] ^ S[(i + 1) % 6] for i in range(6)]
    nocc = S[0] | S[1] | S[2] | S[3] | S[4] | S[5]
    return S, cs, nocc, nocc & ~occ


def push_step(occ, x):
    _, cs, _, allowed = gates(occ)
    return allowed & (up(x & cs[2]) | down(x & cs[5]) | right((x & cs[0]) | up(x & cs[1])) | left((x & cs[3]) | down(x & cs[4])))


def pull_boards(occ):
    _, cs, _, allowed = gates(occ)
    return [cs[0] & left(allowed), up(cs[1]) & left(allowed), up(cs[2]) & allowed,
            cs[3] & right(allowed), down(cs[4]) & right(allowed), down(cs[5]) & allowed]


def pull_step(occ, x):
    P = pull_boards(occ)
    u, d = up(x), down(x)
    return (u & P[2]) | (d & P[5]) | right((x & P[0]) | (u & P[1])) | left((x & P[3]) | (d & P[4]))


def cell_step(occ, x):
    """The gate rule cell by cell (k == 1: exactly one flank occupied; the target is empty and touches the hive)."""
    out = np.zeros((N, N), dtype=bool)
    for j, c in zip(*np.nonzero(x)):
        for i, (dj, dc) in enumerate(DIRS):
            f1 = ((j + DIRS[i - 1][0]) % N, (c + DIRS[i - 1][1]) % N)
            f2 = ((j + DIRS[(i + 1) % 6][0]) % N, (c + DIRS[(i + 1) % 6][1]) % N)
            t = ((j + dj) % N, (c + dc) % N)
            if occ[f1] != occ[f2] and not occ[t] and any(occ[(t[0] + a) % N, (t[1] + b) % N] for a, b in DIRS):
                out[t] = True
    return out


def to_words(x):
    """bool[12][12] -> the six memory words of a board (word r = rows 2r | 2r+1 << 16, column c = bit c)"""
    rows = (x.astype(np.uint32) << np.arange(N, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    return (rows[0::2] | (rows[1::2] << np.uint32(16))).astype(np.uint32)


def from_words(w):
    rows = np.empty(N, dtype=np.uint32)
    rows[0::2] = w & np.uint32(0xFFFF)
    rows[1::2] = w >> np.uint32(16)
    return ((rows[:, None] >> np.arange(N, dtype=np.uint32)) & 1).astype(bool)


def cells(*rc):
    x = np.zeros((N, N), dtype=bool)
    for j, c in rc:
        x[j % N, c % N] = True
    return x


def random_occ(rng, k):
    x = np.zeros(N * N, dtype=bool)
    x[rng.choice(N * N, size=k, replace=False)] = True
    return x.reshape(N, N)


# ------------------------------------------------------------------ no GPU: the algebra
def test_words_round_trip():
    rng = np.random.default_rng(5)
    x = random_occ(rng, 50)
    assert np.array_equal(from_words(to_words(x)), x)
    assert to_words(cells((0, 0)))[0] == 1 and to_words(cells((1, 11)))[0] == 1 << 27 and to_words(cells((11, 0)))[5] == 1 << 16


def test_pull_form_equals_push_form_and_the_cell_model():
    rng = np.random.default_rng(20)
    for case in range(600):
        occ = random_occ(rng, int(rng.integers(1, 41)))
        if case % 3 == 0:
            x = cells(divmod(int(rng.integers(N * N)), N))
        elif case % 3 == 1:
            x = random_occ(rng, int(rng.integers(1, 144)))
        else:
            x = gates(occ)[3]              # every empty cell touching the hive
        a, b = push_step(occ, x), pull_step(occ, x)
        assert np.array_equal(a, b), case
        if case < 150:
            assert np.array_equal(a, cell_step(occ, x)), case


def test_set_up_identities():
    rng = np.random.default_rng(21)
    for _ in range(300):
        occ = random_occ(rng, int(rng.integers(1, 41)))
        S, cs, _, _ = gates(occ)
        assert np.array_equal(up(cs[2]), cs[5]) and np.array_equal(down(cs[5]), cs[2])
        assert np.array_equal(up(cs[1]), up(S[0]) ^ occ)
        assert np.array_equal(down(cs[4]), down(S[3]) ^ occ)
        # as make_pull_ctx forms them: up(S0) = left(S5), down(S3) = right(S2)
        assert np.array_equal(up(S[0]), left(S[5])) and np.array_equal(down(S[3]), right(S[2]))


def test_beetle_step_one_flank_or_none_is_not_both_and_touching():
    """piece_dests' Beetle rule: (k == 1 steps) | (k == 0 steps onto cells touching the hive) == (steps that are not
    k == 2) & touching -- a k == 1 step ends next to its occupied flank."""
    rng = np.random.default_rng(22)

    def shift_dirs(a):
        return up(a[2]) | down(a[5]) | right(a[0] | up(a[1])) | left(a[3] | down(a[4]))
    for _ in range(300):
        occ = random_occ(rng, int(rng.integers(1, 41)))
        x = cells(divmod(int(rng.integers(N * N)), N))
        S, cs, nocc, _ = gates(occ)
        both = [S[(i - 1) % 6] & S[(i + 1) % 6] for i in range(6)]
        q1 = shift_dirs([x & cs[i] for i in range(6)])
        q0 = shift_dirs([x & ~cs[i] & ~both[i] for i in range(6)])
        assert np.array_equal(q1 | (q0 & nocc), shift_dirs([x & ~both[i] for i in range(6)]) & nocc)


# ------------------------------------------------------------------ GPU: the two device forms, both lane layouts
@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible GPU")
    import hive_alphazero_amd as h
    return h.load()


def _golden_occupancies(golden_games, count):
    """occupancies of reference positions, spread over the games, densest plies first"""
    out = []
    for gm in golden_games:
        rec = max(gm["plies"], key=lambda r: sum(p != 255 for p in r["pos"]))
        occ = np.zeros((N, N), dtype=bool)
        for p in rec["pos"]:
            if p != 255:
                occ[p // N, p % N] = True
        out.append(occ)
        if len(out) == count:
            break
    assert len(out) == count
    return out


def _moved_to(occ, target):
    """occ translated on the torus so that one of its cells with a non-empty slide step lands on `target`; the source set"""
    _, _, _, allowed = gates(occ)
    for j, c in zip(*np.nonzero(allowed)):
        if cell_step(occ, cells((j, c))).any():
            sh = ((target[0] - j) % N, (target[1] - c) % N)
            return np.roll(occ, sh, axis=(0, 1)), cells(target)
    raise AssertionError("no cell of this occupancy can slide")


@pytest.fixture(scope="module")
def step_cases(golden_games):
    """32 (occupancy, source set) pairs; the first 16 alone already hold every kind of case."""
    g = _golden_occupancies(golden_games, 24)
    rng = np.random.default_rng(23)
    full, empty = np.ones((N, N), dtype=bool), np.zeros((N, N), dtype=bool)
    case = []
    # single source cells on the lane seams of the quad (rows 3/4, 7/8) and the pair (5/6), the torus wrap (rows 0, 11)
    # and the first and last column
    for k, t in enumerate([(0, 0), (3, 11), (4, 0), (5, 11), (6, 0), (7, 11), (8, 0), (11, 11), (0, 11), (11, 0)]):
        case.append(_moved_to(g[k], t))
    case.append((empty, full))                         # an empty board: nothing touches a hive
    case.append((cells((0, 0)), full))                 # one piece in the corner: its ring wraps both ways
    case.append((g[10], full))
    case += [(g[k], gates(g[k])[3]) for k in (11, 12, 13)]
    assert len(case) == 16
    for k, t in enumerate([(3, 0), (4, 11), (5, 0), (6, 11), (7, 0), (8, 11)]):
        case.append(_moved_to(g[14 + k], t))
    case.append((cells((11, 11)), cells((0, 0))))      # one piece, one source across the wrap
    case.append((empty, cells((6, 6))))
    case += [(g[k], full) for k in (20, 21)]
    case += [(g[k], random_occ(rng, 30)) for k in (22, 23, 0, 1)]
    case += [(np.roll(g[k], (5, 7), axis=(0, 1)), gates(np.roll(g[k], (5, 7), axis=(0, 1)))[3]) for k in (2, 3)]
    assert len(case) == 32
    want = [cell_step(o, x) for o, x in case]
    for o, x in case:
        assert np.array_equal(push_step(o, x), pull_step(o, x))
    # the single-cell cases do step, and the expected boards reach over every seam and the wrap
    assert all(w.any() for w in want[:10]) and all(w.any() for w in want[16:22])
    seen = np.zeros((N, N), dtype=bool)
    for w in want:
        seen |= w
    assert seen[[0, 3, 4, 5, 6, 7, 8, 11]].any(axis=1).all() and seen[:, [0, 11]].any(axis=0).all()
    return case, want


def test_step_cases_cover_the_seams(step_cases):
    case, want = step_cases          # (the fixture asserts the coverage; this runs it without a GPU as well)
    assert len(case) == len(want) == 32


def _device_step(lib, cases, pair):
    import torch
    occ = torch.from_numpy(np.stack([to_words(o) for o, _ in cases]).view(np.int32)).cuda()
    src = torch.from_numpy(np.stack([to_words(x) for _, x in cases]).view(np.int32)).cuda()
    push = torch.full_like(occ, -1)
    pull = torch.full_like(occ, -1)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.hive_debug_slide_step(P(occ), P(src), len(cases), pair, P(push), P(pull), None) == 0
    torch.cuda.synchronize()
    return push.cpu().numpy().view(np.uint32), pull.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [0, 1], ids=["quad16", "pair32"])
def test_device_pull_step_equals_push_step_and_model(lib, step_cases, pair):
    case, want = step_cases
    batches = [(0, 32)] if pair else [(0, 16), (16, 32)]       # one full wave per launch in either layout
    for lo, hi in batches:
        push, pull = _device_step(lib, case[lo:hi], pair)
        exp = np.stack([to_words(w) for w in want[lo:hi]])
        assert np.array_equal(push, pull)
        assert np.array_equal(pull, exp)


@pytest.mark.gpu
def test_debug_slide_step_refuses_bad_arguments(lib):
    import torch
    t = torch.zeros(6, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.hive_debug_slide_step(p, p, 0, 0, p, p, None) == -1
    assert lib.hive_debug_slide_step(None, p, 1, 0, p, p, None) == -1


# ------------------------------------------------------------------ GPU: the legal-move launch against the CPU oracle
@pytest.fixture(scope="module")
def corpus():
    """33 mid-game positions of seeded oracle playouts with their legal sets."""
    from oracle import oracle_py as O
    rng = np.random.default_rng(31)
    turn, pos, lvl, mode, legal = [], [], [], [], []
    while len(turn) < 33:
        g = O.OracleGame()
        ply = 0
        while len(turn) < 33:
            acts = g.actions()
            over, _ = g.game_is_over()
            if over or g.turn >= 55:
                break
            if ply >= 12 and ply % 3 == 0:
                p, l = g.pieces()
                turn.append(g.turn); pos.append(p); lvl.append(l); mode.append(g.nmt_mode); legal.append(acts)
            g.move(int(acts[rng.integers(len(acts))]) if acts else -1)
            ply += 1
    turn, pos = np.array(turn), np.array(pos)
    # movable Ants and Spiders of the side to move (action id = cell * 11 + slot; Spiders are slots 3-4, Ants 8-10)
    movable = {"spider": 0, "ant": 0}
    for t, p, acts in zip(turn, pos, legal):
        stm = 0 if t & 1 else 1
        for slot in range(3, 11):
            if slot in (3, 4, 8, 9, 10) and p[stm * 11 + slot] != 255 and any(a % 11 == slot for a in acts):
                movable["spider" if slot < 5 else "ant"] += 1
    assert movable["spider"] >= 3 and movable["ant"] >= 3, movable
    return turn, pos, np.array(lvl), np.array(mode, dtype=np.uint8), legal


def test_corpus_has_movable_ants_and_spiders(corpus):
    assert len(corpus[4]) == 33


@pytest.mark.gpu
@pytest.mark.parametrize("pair,sizes", [(False, (1, 16, 17)), (True, (1, 32, 33))], ids=["quad", "pair"])
def test_movegen_vs_oracle_around_one_wave(lib, corpus, pair, sizes):
    import torch
    from hive_alphazero_amd import batch, packing
    turn, pos, lvl, mode, legal = corpus
    boards = torch.from_numpy(packing.pack_boards(turn, pos, lvl, mode)).cuda()
    lib.hive_movegen_pair_threshold(1 if pair else 1 << 30)
    try:
        for n in sizes:
            for want_list in (False, True):
                mask, count, lst = batch.movegen(boards[:n].contiguous(), want_list=want_list)
                torch.cuda.synchronize()
                m = mask.cpu().numpy().view(np.uint32)
                assert [packing.mask_to_actions(r) for r in m] == legal[:n], (n, want_list)
                assert count.cpu().numpy().tolist() == [len(x) for x in legal[:n]]
                if want_list:
                    l = lst.cpu().numpy()
                    for i in range(n):
                        assert l[i, :len(legal[i])].tolist() == legal[i] and np.all(l[i, len(legal[i]):] == -1)
    finally:
        lib.hive_movegen_pair_threshold(0)
