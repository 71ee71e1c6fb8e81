"""GPU parity at the places the centre-of-the-board playouts do not reach: every position on all 144 torus translates (the
Grasshopper's legal set depends on where the hive sits: DESIGN.md), the true reference's games at the board's seam, tall
stacks, finished games and zero-legal positions, in every movegen instantiation.  Bit-exact against the CPU oracle and the
golden games; tests/test_env_corpus_host.py asserts the coverage of the inputs on the oracle alone."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import env_corpus as E
from test_gpu_env import GOLD, _golden_positions, hv, lockstep_vs_oracle, replay_games   # noqa: F401  (hv is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def expected_words(masks):
    """uint8[n,1584] legal masks (id = cell*11 + slot) -> int32[n,66] destination boards as the kernel writes them."""
    n = masks.shape[0]
    m = masks.reshape(n, 12, 12, 11).transpose(0, 3, 1, 2).astype(np.uint32)            # [n, slot, row, col]
    rows = (m << np.arange(12, dtype=np.uint32)).sum(axis=3, dtype=np.uint32)           # [n, slot, row]
    return (rows[:, :, 0::2] | (rows[:, :, 1::2] << np.uint32(16))).reshape(n, 66).view(np.int32)


def expected_lists(masks):
    """-> int16[n,256]: the ascending legal ids of each row, -1 padded (the first 256 of a longer set)."""
    n = masks.shape[0]
    rows, ids = np.nonzero(masks)
    count = masks.sum(axis=1, dtype=np.int64)
    rank = np.arange(len(rows)) - np.repeat(np.cumsum(count) - count, count)
    out = np.full((n, 256), -1, dtype=np.int16)
    keep = rank < 256
    out[rows[keep], rank[keep]] = ids[keep]
    return out


def masks_of(legal_lists):
    masks = np.zeros((len(legal_lists), 1584), dtype=np.uint8)
    for i, ids in enumerate(legal_lists):
        masks[i, ids] = 1
    return masks


class Expected:
    """What movegen must return for a set of boards, on the GPU, and the comparison with a readable failure."""

    def __init__(self, packing, turn, pos, lvl, mode, masks):
        self.masks = masks
        self.boards = torch.from_numpy(packing.pack_boards(turn, pos, lvl, mode)).cuda()
        self.words = torch.from_numpy(expected_words(masks)).cuda()
        self.count = torch.from_numpy(masks.sum(axis=1, dtype=np.int32)).cuda()
        self.lists = torch.from_numpy(expected_lists(masks)).cuda()
        for i in range(0, len(masks), max(1, len(masks) // 5)):                           # the helpers against packing.py
            assert np.array_equal(packing.actions_to_mask(np.nonzero(masks[i])[0]).view(np.int32), self.words[i].cpu().numpy())

    def check(self, batch, n=None, want_list=True, what=""):
        from hive_alphazero_amd import packing
        n = len(self.masks) if n is None else n
        mask, count, lst = batch.movegen(self.boards[:n].contiguous(), want_list=want_list)
        bad = (mask != self.words[:n]).any(dim=1).nonzero().view(-1).cpu().tolist()
        for i in bad[:5]:
            got, want = set(packing.mask_to_actions(mask[i].cpu().numpy().view(np.uint32))), set(np.nonzero(self.masks[i])[0].tolist())
            print(f"{what}: board {i} (position {i // 144}, offset {E.OFFSETS[i % 144]}): slots {sorted({a % 11 for a in got ^ want})}"
                  f" extra {sorted(got - want)} missing {sorted(want - got)}")
        assert not bad, f"{what}: {len(bad)} of {n} boards differ"
        assert torch.equal(count, self.count[:n]), what
        if want_list:
            assert torch.equal(lst, self.lists[:n]), what        # ascending, -1 padded, equal to the mask


def with_pair_threshold(L, threshold, fn):
    L.hive_movegen_pair_threshold(threshold)
    try:
        fn()
    finally:
        L.hive_movegen_pair_threshold(0)
    assert L.hive_movegen_pair_threshold(-1) == 16384


@pytest.fixture(scope="module")
def translated(hv):
    """256 positions x 144 offsets with the oracle's legal sets, computed once."""
    from oracle import oracle_py as O
    corpus = E.translated_corpus()
    boards = E.translated_boards(corpus)
    _, masks = O.batch_legal(*boards)
    return corpus, Expected(hv[2], *boards, masks)


@pytest.fixture(scope="module")
def seam_games():
    with gzip.open(os.path.join(GOLD, "games_seam.json.gz"), "rt") as f:
        return json.load(f)["games"]


def test_movegen_on_all_translates(hv, translated):
    """36,864 boards, both lane layouts, with and without the fused id list, and a ragged pair-layout prefix."""
    h, batch, packing = hv
    L = h.load()
    corpus, exp = translated
    assert len(exp.masks) == 36864 >= L.hive_movegen_pair_threshold(-1) == 16384           # the default picks the pair layout
    for want_list in (True, False):
        exp.check(batch, want_list=want_list, what=f"default threshold, list={want_list}")
        with_pair_threshold(L, 1 << 30, lambda: exp.check(batch, want_list=want_list, what=f"quad layout, list={want_list}"))
        with_pair_threshold(L, 1, lambda: exp.check(batch, n=145, want_list=want_list, what=f"pair layout, 145 boards, list={want_list}"))


def test_seam_games_replay_and_flat_movegen(hv, seam_games):
    """The true reference's games at the seam: ply by ply through BoardBatch, and every position through the stateless
    movegen in both layouts."""
    h, batch, packing = hv
    L = h.load()
    replay_games(hv, seam_games)
    recs, turn, pos, lvl, mode = _golden_positions(seam_games)
    exp = Expected(packing, turn, pos, lvl, mode, masks_of([r["legal"] for r in recs]))
    with_pair_threshold(L, 1, lambda: exp.check(batch, what="games_seam, pair layout"))
    with_pair_threshold(L, 1 << 30, lambda: exp.check(batch, what="games_seam, quad layout"))


def test_biased_playouts_vs_oracle_lockstep(hv):
    """The lock-step comparison under drift, stack and crowd, 96 games each; the run checks that it did reach tall stacks,
    finished games of both winners and zero-legal positions."""
    policies = ["drift", "stack", "crowd"]
    rng = np.random.default_rng(21)
    direction = [E.DRIFT_DIRS[rng.integers(len(E.DRIFT_DIRS))] for _ in range(288)]
    stack = np.zeros(8, dtype=np.int64)
    finished = {0: 0, 1: 0, 2: 0}
    zero_legal = [0]

    def pick(i, g, legal):
        pos, lvl = g.pieces()
        return E.choose(policies[i % 3], E.Position(g.turn, pos, lvl, g.nmt_mode, legal, False, 0), rng, direction[i])

    def seen(g, legal, over, winner):
        pos, lvl = g.pieces()
        stack[int(lvl[pos != 255].max()) if (pos != 255).any() else 0] += 1
        zero_legal[0] += not legal
        if over:
            finished[winner] += 1

    lockstep_vs_oracle(hv, 288, rng, pick, seen)
    print("biased lock-step:", int(stack.sum()), "positions; highest stack index histogram", stack.tolist(), "; finished by winner",
          finished, "; draws", finished[0], "; zero-legal positions", zero_legal[0])
    assert stack[3:].sum() >= 30 and stack[4:].sum() >= 1
    assert sum(finished.values()) >= 40 and finished[1] > 0 and finished[2] > 0
    assert zero_legal[0] >= 5


def test_terminal_on_all_translates(hv):
    """64 finished crowd positions of both winners and the position one ply before each, at all 144 offsets."""
    h, batch, packing = hv
    from oracle import oracle_py as O
    L = h.load()
    pairs = E.finished_with_previous(64, seed=14)
    positions = [p for pair in pairs for p in pair]
    assert sum(p.over for p in positions) == 64 and {p.winner for p in positions if p.over} == {1, 2}
    turn, pos, lvl, mode = E.translated_boards(positions)
    want = np.array([O.OracleGame.from_position(int(t), p, l, 0).game_is_over() for t, p, l in zip(turn, pos, lvl)], dtype=np.int8)
    assert want[:, 0].reshape(128, 144).all(axis=1).tolist() == [p.over for p in positions]   # surrounded is translation-invariant
    boards = torch.from_numpy(packing.pack_boards(turn, pos, lvl, mode)).cuda()
    n = len(turn)
    over = torch.full((n,), -7, dtype=torch.int8, device="cuda")
    winner = torch.full((n,), -7, dtype=torch.int8, device="cuda")
    assert L.hive_terminal_launch(_P(boards), n, _P(over), _P(winner), None) == 0
    torch.cuda.synchronize()
    over, winner = over.cpu().numpy(), winner.cpu().numpy()
    bad = np.nonzero((over != want[:, 0]) | (winner != want[:, 1]))[0]
    for i in bad[:5]:
        print(f"terminal: position {i // 144} offset {E.OFFSETS[i % 144]}: got {over[i], winner[i]} want {tuple(want[i])}")
    assert len(bad) == 0, f"{len(bad)} of {n} boards differ"


def test_leaf_launch_equals_separate_launches(hv, translated):
    """hive_leaf_launch (planes + legal set + terminal in one call, its own movegen instantiation) on every ninth board of
    the translated corpus (4,096 boards: all 256 positions at 16 offsets each) with random histories."""
    h, batch, packing = hv
    from hive_alphazero_amd._lib import BF16, HIVE_MASK_WORDS, HWC
    L = h.load()
    corpus, exp = translated
    n = 4096
    pickb = torch.arange(n, device="cuda") * 9
    boards = exp.boards[pickb].contiguous()
    g = torch.Generator(device="cuda").manual_seed(5)
    hist = torch.randint(0, 256, (n, 384), dtype=torch.uint8, device="cuda", generator=g)
    hist[:, 1::4] &= 0x0F
    hist[:, 3::4] &= 0x0F                                                             # 12-bit rows in 16-bit fields
    boards[:, 35] = torch.randint(0, 5, (n,), dtype=torch.uint8, device="cuda", generator=g) * 17   # history lengths 0..4 / 0..4
    ws = torch.empty((n * 144,), dtype=torch.int64, device="cuda")
    planes = torch.full((n, 12, 12, 56), float("nan"), dtype=torch.bfloat16, device="cuda")
    mask = torch.full((n, HIVE_MASK_WORDS), -1, dtype=torch.int32, device="cuda")
    count = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    over = torch.full((n,), -7, dtype=torch.int8, device="cuda")
    winner = torch.full((n,), -7, dtype=torch.int8, device="cuda")
    assert L.hive_leaf_launch(_P(boards), _P(hist), n, _P(planes), BF16, HWC, _P(ws), _P(mask), _P(count), _P(over), _P(winner), None) == 0
    m2, c2, _ = batch.movegen(boards)
    o2, w2 = torch.full_like(over, -5), torch.full_like(winner, -5)
    assert L.hive_terminal_launch(_P(boards), n, _P(o2), _P(w2), None) == 0
    p2 = torch.full_like(planes, float("nan"))
    ws2 = torch.empty_like(ws)
    assert L.hive_encode_launch(_P(boards), _P(hist), n, _P(p2), BF16, HWC, _P(ws2), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(mask, m2) and torch.equal(count, c2)
    assert torch.equal(mask, exp.words[pickb]) and torch.equal(count, exp.count[pickb])          # and both equal the oracle
    assert torch.equal(over, o2) and torch.equal(winner, w2) and int(over.min()) >= 0
    assert torch.equal(planes.view(torch.int16), p2.view(torch.int16)) and torch.equal(ws, ws2)
    assert bool(torch.isfinite(planes.float()).all())
