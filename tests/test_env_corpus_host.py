"""CPU-only: the oracle against the true reference's games at the board's seam (tests/golden/games_seam.json.gz), and the
coverage that the GPU tests of tests/test_gpu_env_seam.py lean on, asserted on the oracle alone -- so a GPU test can never
pass by having skipped the hard cases."""
import gzip
import json
import os

import numpy as np
import pytest

import env_corpus as E
from oracle import oracle_py as O
from test_oracle_golden import _check_ply

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEAM = os.path.join(GOLD, "games_seam.json.gz")


@pytest.fixture(scope="module")
def seam_games():
    with gzip.open(SEAM, "rt") as f:
        return json.load(f)["games"]


@pytest.fixture(scope="module")
def corpus():
    return E.translated_corpus()


def test_oracle_replays_seam_games(seam_games):
    """State, legal ids, nmt, planes, over / winner and key of every ply, through move and through from_position."""
    npos = 0
    for gm in seam_games:
        assert gm["policy"] == "drift"
        g = O.OracleGame()
        for i, rec in enumerate(gm["plies"]):
            ctx = f"seed {gm['seed']} ply {i}"
            _check_ply(g, rec, ctx)
            p = E.from_record(rec)
            h = O.OracleGame.from_position(p.turn, p.pos, p.lvl, p.mode)
            assert h.actions() == rec["legal"], ctx
            assert h.nmt() == rec["nmt"], ctx
            assert h.game_is_over() == (rec["over"], rec["win"]), ctx
            assert h.state_key() == rec["key"], ctx
            npos += 1
            if rec["a"] is not None:
                g.move(rec["a"])
    assert npos > 2000


def test_seam_fixture_lives_at_the_seam(seam_games):
    assert os.path.getsize(SEAM) <= os.path.getsize(os.path.join(GOLD, "games_full.json.gz")) <= 370289
    plies = [E.from_record(rec) for gm in seam_games for rec in gm["plies"]]
    c = E.coverage(plies)
    assert int((c["cells"] == 0).sum()) == 0, np.nonzero(c["cells"] == 0)[0].tolist()
    assert c["seam_touch"] >= 0.60 * c["mode0"], (c["seam_touch"], c["mode0"])
    shows = E.seam_rule([p for p in plies if p.mode == 0], stop_at=150)
    print("games_seam:", len(plies), "plies,", c["seam_touch"], "of", c["mode0"], "mode-0 plies touch the seam, least-visited cell",
          int(c["cells"].min()), "plies; the seam rule shows in", int(shows.sum()), "(counting stopped at 150)")
    assert shows.sum() >= 150


def test_translated_corpus_coverage(corpus):
    """The input conditions of the translated-movegen test."""
    c = E.coverage(corpus)
    assert len(corpus) == 256 and c["mode0"] == 256
    assert c["stack"][3:].sum() >= 20, c["stack"]
    assert c["zero_legal"] >= 4
    assert min(c["to_move"]) >= 64, c["to_move"]
    # translate() is a bijection of the cells that keeps pieces in hand, and offset (0, 0) is the identity
    p = corpus[0]
    assert np.array_equal(E.translate(p.pos, 0, 0), p.pos)
    assert np.array_equal(E.translate(E.translate(p.pos, 5, 11), 7, 1), p.pos)
    assert E.translate(np.array([0, 143, 255, 11], dtype=np.uint8), 1, 1).tolist() == [13, 0, 255, 12]


def test_grasshopper_is_the_only_piece_that_sees_the_seam(corpus):
    """The seam fact: over the 256 x 144 translated boards, a board whose legal set is not the translate of its base
    position's differs from it in slots 5-7 (the Grasshoppers) only, and such boards are at least a tenth of all."""
    total, masks = O.batch_legal(*E.translated_boards(corpus))
    assert total == int(masks.sum())
    base = E.untranslate_masks(masks)                          # [256, 144 offsets, 144 cells, 11 slots]
    for i, p in enumerate(corpus):
        assert np.nonzero(base[i, 0].reshape(-1))[0].tolist() == p.legal
    differs = base != base[:, :1]
    boards = differs.any(axis=(2, 3))
    by_slot = differs.sum(axis=(0, 1, 2))
    extra = int((differs & (base == 1)).sum())
    missing = int((differs & (base == 0)).sum())
    print("translated corpus:", int(boards.sum()), "of", boards.size, "boards differ from their base's translate;",
          extra, "extra and", missing, "missing ids; by slot", by_slot.tolist())
    assert by_slot[:5].sum() == 0 and by_slot[8:].sum() == 0
    assert boards.sum() >= 0.10 * boards.size


def test_biased_playouts_reach_the_rare_states():
    """What the policies are for, on 3,000 positions each (the GPU lock-step test asserts its own run's coverage)."""
    c = E.coverage(E.playout("stack", 3000, seed=11))
    assert c["stack"][3] >= 60 and c["stack"][4] >= 3, c["stack"]
    c = E.coverage(E.playout("crowd", 3000, seed=12))
    assert c["finished"][1] >= 20 and c["finished"][2] >= 20, c["finished"]
    drift = E.playout("drift", 3000, seed=13)
    c = E.coverage(drift)
    assert c["seam_touch"] >= 0.60 * c["mode0"], (c["seam_touch"], c["mode0"])
    pairs = E.finished_with_previous(64, seed=14)
    assert len(pairs) == 64 and {b.winner for _, b in pairs} == {1, 2}
    assert all(b.over and not a.over and a.turn + 1 == b.turn for a, b in pairs)
