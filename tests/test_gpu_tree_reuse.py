"""Trees kept across plies (hive_search_advance_roots, TreeSearch(keep_tree=True)): the carried tree is the old subtree
bit for bit, a search from it equals the sequential player that kept its table, a refused or fresh carry is the plain
search, and self-play records do not depend on the batch a game runs in."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mcts_stub import StubPipe, stub_predict   # noqa: E402

NODE_FIELDS = ("nedge", "sum_n", "term")
EDGE_FIELDS = ("act", "n_visits")


def _host_stub_evaluator(planes):
    x = planes.float().cpu().numpy()
    ps, vs = zip(*(stub_predict(x[i]) for i in range(x.shape[0])))
    return torch.from_numpy(np.stack(ps)).cuda(), torch.tensor(vs, dtype=torch.float32).cuda()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _canonical(tree, start):
    """The nodes reachable from `start` through child >= 0 in breadth-first edge order: a list of per-node dicts whose
    `child` entries are positions in that list (floats as their bit patterns)."""
    order, index = [start], {start: 0}
    for node in order:
        for e in range(int(tree["nedge"][node])):
            c = int(tree["child"][node, e])
            if c >= 0 and c not in index:
                index[c] = len(order)
                order.append(c)
    out = []
    for node in order:
        ne = int(tree["nedge"][node])
        child = np.array([index[int(c)] if c >= 0 else -1 for c in tree["child"][node, :ne]], dtype=np.int64)
        out.append({"board": tree["board"][node].copy(), "hist": tree["hist"][node].copy(), "nedge": ne,
                    "sum_n": int(tree["sum_n"][node]), "term": int(tree["term"][node]), "tv": _bits(tree["tv"][node:node + 1]),
                    "act": tree["act"][node, :ne].copy(), "n_visits": tree["n_visits"][node, :ne].copy(),
                    "p": _bits(tree["p"][node, :ne]), "w": _bits(tree["w"][node, :ne]), "child": child})
    return out


def _finished_record(golden_games):
    """HiveBoard record of a game that ended by a surrounded queen (19 plies, tests/golden/games_full.json.gz)."""
    from hive_alphazero_amd.env_hive import GamePlay
    plies = golden_games[20]["plies"]
    assert plies[-1]["over"] and plies[-1]["a"] is None
    g = GamePlay(1050, 900)
    for rec in plies[:-1]:
        g.move(rec["a"])
    assert g.game_is_over()
    return np.asarray(g._rec, dtype=np.uint8).reshape(64)


@pytest.mark.parametrize("merge", [True, False])
def test_carried_tree_is_the_old_subtree_bit_for_bit(merge, golden_games):
    """37 positions (no multiple of the 4 games per workgroup): every ply 1..36 of one random playout -- from the opening
    to positions with 100+ legal moves, so kept nodes need more than one 64-lane pass -- and, as no playout of
    playout.random_positions ends within 37 positions, a finished game from the golden corpus as the 37th.  32 simulations
    with noise, export, step, advance, export: the kept tree is the closure of the played child, every field equal bit
    for bit, node 0 carrying the stepped position; games that do not carry come out as hive_search_set_roots leaves them
    and their next search is the plain search."""
    assert torch.cuda.is_available()
    from hive_alphazero_amd import batch, mcts, playout
    G, sims = 37, 32
    pos = playout.random_positions(G, seed=5, games=1).clone()
    pos[G - 1] = torch.from_numpy(_finished_record(golden_games)).to(pos.device)
    B = batch.BoardBatch(G)
    B.import_state(pos)
    rb, rh = B.export_state()
    over = B.terminal()[0].cpu().numpy()
    assert over[G - 1] == 1 and over[:G - 1].sum() == 0
    UNRELATED, UNVISITED, IDLE, IDLE_LATER, OVER = 3, 10, 7, 9, G - 1      # (position 10 has more legal moves than simulations)
    active = torch.ones((G,), dtype=torch.int8, device="cuda")
    active[IDLE] = 0
    ts = mcts.TreeSearch(G, sims, _host_stub_evaluator, plane_dtype=torch.float32, seed=3, keep_tree=True, transpositions=merge)
    assert ts.max_nodes == 3 * sims + 1 + 2
    action, _, sum_n = ts.search(rb, rh, active=active)
    kept0, visits0, refused0 = (x.cpu().numpy() for x in ts.carry_stats())
    assert not kept0.any() and not visits0.any() and not refused0.any()          # nothing to carry into a first search
    before = [ts.export_tree(g) for g in range(G)]
    step = action.cpu().numpy().copy()
    assert step[IDLE] == -2 and step[OVER] == -2 and (np.delete(step, [IDLE, OVER]) >= -1).all()
    # one game plays a root edge the search never went through
    root = before[UNVISITED]
    unvisited = [e for e in range(int(root["nedge"][0])) if root["child"][0, e] == -1 and root["n_visits"][0, e] == 0]
    step[UNVISITED] = int(root["act"][0, unvisited[0]])
    played = np.where(step == -2, -3, step).astype(np.int32)
    played[UNRELATED] = -3
    played[OVER] = -1               # "a pass was played" from a finished game: the old root is a terminal node, nothing carries
    B.step(torch.from_numpy(step).cuda())
    assert B.illegal_count() == 0
    rb2, rh2 = B.export_state()
    active2 = active.clone()
    active2[IDLE_LATER] = 0
    ts.advance_roots(rb2, rh2, active=active2, played=torch.from_numpy(played).cuda())
    kept, visits, refused = (x.cpu().numpy() for x in ts.carry_stats())
    after = [ts.export_tree(g) for g in range(G)]
    boards2, hist2 = rb2.cpu().numpy(), rh2.cpu().numpy()
    fresh = {UNRELATED, UNVISITED, IDLE, IDLE_LATER, OVER}
    carried, wide = 0, 0
    for g in range(G):
        old, new = before[g], after[g]
        child = -1
        if g not in fresh:
            edge = [e for e in range(int(old["nedge"][0])) if old["act"][0, e] == played[g]]
            assert len(edge) == 1
            child = int(old["child"][0, edge[0]])
            if child >= 0 and old["term"][child]:
                child = -1
        if child < 0:
            assert new["n"] == 0 and kept[g] == 0 and visits[g] == 0, g
            continue
        want, got = _canonical(old, child), _canonical(new, 0)
        assert new["n"] == len(want) == len(got) == kept[g], g
        assert visits[g] == old["sum_n"][child], g
        assert np.array_equal(got[0]["board"], boards2[g]) and np.array_equal(got[0]["hist"], hist2[g]), g
        for k, (a, b) in enumerate(zip(want, got)):
            for f in NODE_FIELDS:
                assert a[f] == b[f], (g, k, f)
            for f in ("tv", "p", "w", "child") + EDGE_FIELDS + (("board", "hist") if k else ()):
                assert np.array_equal(a[f], b[f]), (g, k, f)
        assert not any((n["child"] < -1).any() for n in got)
        carried += 1
        wide += sum(n["nedge"] > 64 for n in got)
    assert not refused.any()
    assert carried >= G - len(fresh) - 2 and wide > 0          # kept nodes with more than one lane pass of edges
    # the next search: carried visits stay in the root; the trees that did not carry search like a plain TreeSearch
    a2, p2, n2 = ts.run_simulations()
    plain = mcts.TreeSearch(G, sims, _host_stub_evaluator, plane_dtype=torch.float32, seed=3, transpositions=merge)
    a1, p1, n1 = plain.search(rb2, rh2, active=active2)
    for g in range(G):
        if kept[g] == 0:
            assert a2[g].item() == a1[g].item() and n2[g].item() == n1[g].item() and torch.equal(p2[g], p1[g]), g
        else:
            assert n2[g].item() == visits[g] + sims, g
    assert a2[IDLE].item() == -2 and a2[IDLE_LATER].item() == -2 and a2[OVER].item() == -2
    ts.close(); plain.close(); B.close()


def _mirror_and_gpu(prefix_seed, plies, sims, moves):
    """`moves` consecutive searches of the sequential HivePlayer(keep_tree=True) and of TreeSearch(keep_tree=True) from
    one position, the mirror's move played in both; yields (mirror root edges {action: n}, mirror root sum_n,
    GPU root edges, GPU sum_n, GPU transposition hits so far) per move."""
    import hive_alphazero_amd.solo_play as sp
    from hive_alphazero_amd import batch, mcts
    from hive_alphazero_amd.env_hive import GamePlay
    rng = np.random.default_rng(prefix_seed)
    g = GamePlay(1050, 900)
    for _ in range(plies):
        acts = g.actions()
        g.move(int(acts[rng.integers(len(acts))]))
    sp.SEARCH_THREADS = 1
    old_eps = sp.noise_eps
    sp.noise_eps = 0.0
    B = batch.BoardBatch(1)
    B.import_state(g._rec.reshape(1, 64), g._hist.reshape(1, 384))
    ts = mcts.TreeSearch(1, sims, _host_stub_evaluator, plane_dtype=torch.float32, noise_eps=0.0, keep_tree=True)
    try:
        player = sp.HivePlayer(pipes=[StubPipe()])
        player.keep_tree = True
        player.simulation_num_per_move = sims
        np.random.seed(0)
        played = None
        for _ in range(moves):
            move, _ = player.action(g)
            entry = player.tree[g.state_key]
            ref = {int(a): int(s.n) for a, s in entry.a.items() if s.n > 0}
            rb, rh = B.export_state()
            _, _, sum_n = ts.search(rb, rh, played=played)
            visits = ts.root_stats()[0][0].cpu().numpy()
            got = {int(a): int(visits[a]) for a in np.nonzero(visits)[0]}
            yield ref, int(entry.sum_n), got, int(sum_n[0].item()), int(ts.transposition_hits()[0].item())
            g.move(move)
            B.step(torch.tensor([move], dtype=torch.int32))
            played = torch.tensor([move], dtype=torch.int32)
        assert B.illegal_count() == 0
    finally:
        sp.noise_eps = old_eps
        ts.close(); B.close()


@pytest.mark.parametrize("prefix_seed,plies", [(22, 3), (23, 8), (24, 14)])
def test_search_from_a_carried_tree_equals_the_sequential_player_that_kept_its_table(prefix_seed, plies):
    sims, totals = 40, []
    for ref, ref_sum, got, sum_n, _ in _mirror_and_gpu(prefix_seed, plies, sims, 4):
        assert got == ref and sum_n == ref_sum
        totals.append(sum_n)
    assert totals[0] == sims - 1 and all(t > sims for t in totals[1:])      # every later search started with carried visits


def test_carried_tree_keeps_merging_transpositions():
    """A transposition-rich position (test_search_merges_transpositions_like_the_reference_dict), 300 simulations, two
    moves: the second search runs on the REBUILT hash table and must still find shared positions like the dict does."""
    hits = []
    for ref, ref_sum, got, sum_n, h in _mirror_and_gpu(45, 32, 300, 2):      # (the mirror counts 5, then 2 more, shared entries)
        assert got == ref and sum_n == ref_sum
        hits.append(h)
    assert hits[1] > hits[0]


def test_refused_or_fresh_carry_is_the_plain_search():
    """max_nodes = sims + slots + 2 leaves no room for any kept node next to a whole search: every carry is refused by the
    pool bound and counted, and both searches equal TreeSearch(keep_tree=False) on the same roots."""
    assert torch.cuda.is_available()
    from hive_alphazero_amd import batch, mcts, playout
    G, sims = 9, 24
    pos = playout.random_positions(21, seed=5, games=1)[12:21].contiguous()
    B = batch.BoardBatch(G)
    B.import_state(pos)
    rb, rh = B.export_state()
    ts = mcts.TreeSearch(G, sims, _host_stub_evaluator, plane_dtype=torch.float32, seed=7, keep_tree=True, max_nodes=sims + 1 + 2)
    plain = mcts.TreeSearch(G, sims, _host_stub_evaluator, plane_dtype=torch.float32, seed=7)
    assert ts.max_nodes == plain.max_nodes
    first = [x.clone() for x in ts.search(rb, rh)]
    assert all(torch.equal(x, y) for x, y in zip(first, plain.search(rb, rh)))
    trees = [ts.export_tree(g) for g in range(G)]
    played = first[0].clone()
    tried = np.zeros(G, dtype=np.int32)
    for g, t in enumerate(trees):
        edge = [e for e in range(int(t["nedge"][0])) if t["act"][0, e] == played[g].item()]
        child = int(t["child"][0, edge[0]])
        tried[g] = int(child >= 0 and not t["term"][child])
    assert tried.sum() >= G - 1
    B.step(played)
    rb2, rh2 = B.export_state()
    second = [x.clone() for x in ts.search(rb2, rh2, played=played)]
    kept, visits, refused = (x.cpu().numpy() for x in ts.carry_stats())
    assert np.array_equal(refused, tried) and not kept.any() and not visits.any()
    assert all(torch.equal(x, y) for x, y in zip(second, plain.search(rb2, rh2)))
    assert B.illegal_count() == 0
    ts.close(); plain.close(); B.close()


def _encode_words(L, boards, hist):
    """The packed feature words of hive_encode_launch for these positions (int64 [n,144])."""
    from hive_alphazero_amd._lib import HWC, dtype_code, ptr, stream_ptr
    n = boards.shape[0]
    planes = torch.empty((n, 12, 12, 56), dtype=torch.float32, device=boards.device)
    words = torch.zeros((n * 144,), dtype=torch.int64, device=boards.device)
    rc = L.hive_encode_launch(ptr(boards), ptr(hist), n, ptr(planes), dtype_code(torch.float32), HWC, ptr(words),
                              stream_ptr(boards.device))
    assert rc == 0
    return words.view(n, 144).cpu().numpy()


def test_selfplay_with_kept_trees_is_batch_independent():
    """Games 0..7 played in an engine of 8 and in one of 16 slots, 16 simulations, 14 plies, trees kept: identical ply
    records, feature words equal to an encode of the position, no illegal move, visits carried."""
    assert torch.cuda.is_available()
    from hive_alphazero_amd import mcts
    plies, runs = 14, {}
    for G in (8, 16):
        sp = mcts.SelfPlay(G, 16, _host_stub_evaluator, seed=11, plane_dtype=torch.float32, game_ids=range(G),
                           search_options={"keep_tree": True})
        log, carried = [], 0
        for ply in range(plies):
            boards, hist = sp.env.export_state()
            words = _encode_words(sp.search.L, boards, hist)
            sp.play_ply()
            kept, visits, refused = (x.cpu().numpy() for x in sp.search.carry_stats())
            assert (kept == 0).all() if ply == 0 else True
            carried += int(visits.sum())
            assert not refused.any()
            row = []
            for g in range(8):
                rec = sp.last_ply_record(g)
                assert rec is not None
                assert np.array_equal(np.asarray(rec[0]).view(np.int64).reshape(-1), words[g]), (G, ply, g)
                row.append(rec)
            log.append(row)
        torch.cuda.synchronize()
        assert sp.env.illegal_count() == 0 and sp.finished == 0 and carried > 0
        sp.close()
        runs[G] = log
    for ply in range(plies):
        for g in range(8):
            a, b = runs[8][ply][g], runs[16][ply][g]
            assert len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)), (ply, g)


def test_selfplay_slot_of_a_retired_game_starts_fresh():
    """Staggered games reach the length cap within a few plies: the slot that takes the next game id starts from an empty
    tree while its neighbours carry theirs."""
    assert torch.cuda.is_available()
    from hive_alphazero_amd import mcts

    def flat_eval(planes):
        n = planes.shape[0]
        return torch.full((n, 1584), 1.0 / 1584, device="cuda"), torch.zeros((n,), device="cuda")

    G = 32
    sp = mcts.SelfPlay(G, 8, flat_eval, seed=4, plane_dtype=torch.float32, keep_records=False,
                       search_options={"keep_tree": True})
    sp.stagger(seed=2)
    retired = 0
    for ply in range(12):
        ids = sp.game_id.clone()
        sp.play_ply()
        kept = sp.search.carry_stats()[0]
        new = sp.game_id != ids
        if ply == 0:
            assert not kept.any()
        else:
            assert not kept[new].any()
            assert kept[~new].any()
        retired += int(new.sum().item())
    assert retired > 0 and sp.env.illegal_count() == 0
    sp.close()


def test_kept_trees_with_four_leaves_in_flight():
    """slots = 4: carry, then search, over 3 plies; after each search every node's sum_n is the sum of its edges' visits
    (every virtual loss was taken back) and no edge is left marked as in flight."""
    assert torch.cuda.is_available()
    from hive_alphazero_amd import batch, mcts, playout
    G, sims, slots = 5, 21, 4
    pos = playout.random_positions(30, seed=9, games=1)[10:30:4].contiguous()
    assert pos.shape[0] == G
    B = batch.BoardBatch(G)
    B.import_state(pos)
    ts = mcts.TreeSearch(G, sims, _host_stub_evaluator, plane_dtype=torch.float32, seed=5, slots=slots, keep_tree=True)
    played, carried = None, 0
    for ply in range(3):
        rb, rh = B.export_state()
        action, _, sum_n = ts.search(rb, rh, played=played)
        kept, visits, refused = (x.cpu().numpy() for x in ts.carry_stats())
        carried += int(kept.sum())
        assert not refused.any()
        for g in range(G):
            t = ts.export_tree(g)
            assert t["n"] >= max(1, kept[g]) and t["n"] <= ts.max_nodes
            for k in range(t["n"]):
                ne = int(t["nedge"][k])
                assert t["sum_n"][k] == t["n_visits"][k, :ne].sum(), (ply, g, k)
                assert (t["child"][k, :ne] >= -1).all() and (t["child"][k, :ne] < t["n"]).all(), (ply, g, k)
            assert sum_n[g].item() == t["sum_n"][0] >= visits[g]
        played = action.clone()
        B.step(played)
    assert carried > 0 and B.illegal_count() == 0
    ts.close(); B.close()


def test_arena_refuses_kept_trees():
    from hive_alphazero_amd import mcts
    with pytest.raises(ValueError):
        mcts.ArenaSearch(2, 4, _host_stub_evaluator, _host_stub_evaluator, torch.zeros((2,), dtype=torch.int8, device="cuda"),
                         keep_tree=True)
