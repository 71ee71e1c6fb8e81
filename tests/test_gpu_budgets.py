"""Per-game simulation budgets (hive_search_set_budgets): a game with budget b in a batch searched to `sims` simulations ends
with the tree TreeSearch(sims=b) gives it, bit for bit -- fresh and kept trees, both search modes, one and several leaves in
flight -- `quiet` switches the root noise off per game, dropped-out games cost the evaluator no rows, and the two kernels
that fill budgets (the playout-cap draw, the arena's unequal sides) equal their numpy statements."""
import ctypes

import numpy as np
import pytest
import torch

from hive_alphazero_amd import mcts

TREE_NODE = ("board", "hist", "nedge", "sum_n", "term", "tv")
TREE_EDGE = ("act", "p", "n_visits", "w", "child")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from hive_alphazero_amd import _lib as m
    return m.load(), m.check


def stub_evaluator(planes):
    """A position's (p, v) from integer hashes of its planes: a pure per-row function, exact, so the same bits in any batch
    at any row."""
    B = planes.shape[0]
    dev = planes.device
    x = planes.reshape(B, 144, 56).to(torch.int64)
    cell = (x * (torch.arange(56, device=dev) * 41 % 103 + 1)).sum(2)                      # [B,144]
    h = (cell * (torch.arange(144, device=dev) * 59 % 89 + 1)).sum(1, keepdim=True)       # [B,1]
    j = torch.arange(1584, device=dev).view(1, -1)
    mix = (h * (2 * j + 1) + cell[:, torch.arange(1584, device=dev) % 144] * 7907) % 1013
    p = (mix.float() + 1.0) / (1584.0 * 507.0)
    v = ((h.view(-1) * 29) % 2001).float() / 1000.0 - 1.0
    return p, v * 0.9


def _roots(n, seed, games, skip):
    """n positions `skip / games` plies and more into random playouts -> (boards, history)."""
    from hive_alphazero_amd import batch, playout
    boards = playout.random_positions(n + skip, seed=seed, games=games)[skip:].contiguous()
    B = batch.BoardBatch(n)
    B.import_state(boards)
    rb, rh = B.export_state()
    B.close()
    return rb, rh


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _outputs(ts, out):
    """(action, policy, sum_n, visits, total_value, priors) of the search just run, cloned."""
    return [x.clone() for x in out] + [x.clone() for x in ts.root_stats()]


def _same_rows(got, want, rows, what):
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a)[rows], _bits(b)[rows]), (what, k)


def _same_tree(a, b, what):
    """export_tree dicts equal array for array: every node field, and of every node's edge rows the first nedge entries
    (floats by their bits)."""
    assert a["n"] == b["n"], what
    for f in TREE_NODE:
        x, y = a[f], b[f]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, f)
    for k in range(a["n"]):
        ne = int(a["nedge"][k])
        for f in TREE_EDGE:
            x, y = a[f][k, :ne], b[f][k, :ne]
            if x.dtype == np.float32:
                x, y = x.view(np.uint32), y.view(np.uint32)
            assert np.array_equal(x, y), (what, k, f)


# ------------------------------------------------------------------------------------------ 1. the invariant
@pytest.mark.gpu
@pytest.mark.parametrize("mode,slots", [(mcts.PUCT, 1), (mcts.PUCT, 3), (mcts.UCT, 1)])
def test_mixed_budgets_equal_homogeneous_searches(mode, slots):
    G, sims, cycle = 12, 16, (1, 2, 5, 9, 16)
    rb, rh = _roots(G, seed=17, games=4, skip=12)
    assert int(rb[:, 33].min()) >= 3
    budget = [cycle[g % len(cycle)] for g in range(G)]
    ids = torch.arange(G, device="cuda") * 5 + 300
    M = sims + slots + 2

    def run(s, budgets=None):
        ts = mcts.TreeSearch(G, s, stub_evaluator, plane_dtype=torch.float32, seed=9, slots=slots, mode=mode, max_nodes=M)
        ts.set_game_ids(ids)
        out = _outputs(ts, ts.search(rb, rh, budgets=budgets))
        return ts, out

    mixed, got = run(sims, torch.tensor(budget, dtype=torch.int32, device="cuda"))
    hist = mixed.leaf_histogram().cpu().numpy()
    assert hist.sum(1).tolist() == budget                       # one histogram entry per simulation a game took part in
    exported = set()
    for b in cycle:
        ref, want = run(b)
        rows = torch.tensor([g for g in range(G) if budget[g] == b], device="cuda")
        assert len(rows) >= 2
        _same_rows(got, want, rows, b)
        assert (got[0][rows] >= -1).all() and (got[2][rows] <= b - 1).all()       # a move; the first simulation opens the root
        if slots == 1:
            assert (got[2][rows] == b - 1).all()                # (several leaves in flight can collide: that visit is taken back)
        g = int(rows[-1])
        _same_tree(mixed.export_tree(g), ref.export_tree(g), (b, g))
        exported.add(g)
        ref.close()
    assert len(exported) == len(cycle)
    if mode == mcts.PUCT:
        # the budgets change the result at all: games cut short differ from their full search
        full, want = run(sims)
        assert any(not torch.equal(got[1][g], want[1][g]) for g in range(G) if budget[g] < sims)
        full.close()
    # a host-side budget above sims is an error; quiet without budgets too
    with pytest.raises(ValueError):
        mixed.search(rb, rh, budgets=[sims + 1] * G)
    with pytest.raises(ValueError):
        mixed.search(rb, rh, quiet=torch.zeros((G,), dtype=torch.int8, device="cuda"))
    # budgets off again: the plain search, from the handle that ran the mixed one
    again = _outputs(mixed, mixed.search(rb, rh))
    plain, want = run(sims)
    _same_rows(again, want, torch.arange(G, device="cuda"), "off")
    mixed.close(); plain.close()


@pytest.mark.gpu
def test_budget_zero_leaves_a_game_without_a_tree():
    G, sims = 6, 4
    rb, rh = _roots(G, seed=19, games=2, skip=8)
    ts = mcts.TreeSearch(G, sims, stub_evaluator, plane_dtype=torch.float32, seed=2)
    action, policy, sum_n = ts.search(rb, rh, budgets=torch.tensor([0, 4, -3, 2, 0, 4], dtype=torch.int32, device="cuda"))
    assert action[[0, 2, 4]].tolist() == [-2, -2, -2] and (action[[1, 3, 5]] >= -1).all()
    assert ts.node_counts().tolist()[0::2] == [0, 0, 0] and not policy[[0, 2, 4]].any()
    assert ts.leaf_histogram().sum(1).tolist() == [0, 4, 0, 2, 0, 4]
    ts.close()


# ------------------------------------------------------------------------------------------ 2. quiet
@pytest.mark.gpu
def test_quiet_switches_the_noise_off_for_that_game_only():
    G, sims = 12, 10
    rb, rh = _roots(G, seed=23, games=4, skip=12)
    ids = torch.arange(G, device="cuda") * 7 + 11
    quiet = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1], dtype=torch.int8, device="cuda")

    def run(eps, **kw):
        ts = mcts.TreeSearch(G, sims, stub_evaluator, plane_dtype=torch.float32, seed=5, slots=2, noise_eps=eps)
        ts.set_game_ids(ids)
        out = _outputs(ts, ts.search(rb, rh, **kw))
        ts.close()
        return out

    got = run(0.25, budgets=torch.full((G,), sims, dtype=torch.int32, device="cuda"), quiet=quiet)
    noisy, still = run(0.25), run(0.0)
    _same_rows(got, still, torch.nonzero(quiet != 0).view(-1), "quiet")
    _same_rows(got, noisy, torch.nonzero(quiet == 0).view(-1), "noisy")
    assert any(not torch.equal(noisy[3][g], still[3][g]) for g in range(G) if quiet[g])      # the noise does change these games


# ------------------------------------------------------------------------------------------ 3. kept trees
@pytest.mark.gpu
def test_budgets_with_kept_trees_over_two_plies():
    from hive_alphazero_amd import batch
    G, sims = 12, 16
    rb, rh = _roots(G, seed=29, games=4, skip=12)
    M = 3 * sims + 1 + 2
    group = [list(range(0, G // 2)), list(range(G // 2, G))]
    plan = [(16, 4), (4, 16)]                                   # per ply: (budget of group 0, budget of group 1)
    ids = torch.arange(G, device="cuda") + 40
    make = lambda: mcts.TreeSearch(G, sims, stub_evaluator, plane_dtype=torch.float32, seed=13, keep_tree=True, max_nodes=M)
    mixed, refs = make(), [make(), make()]
    for ts in [mixed] + refs:
        ts.set_game_ids(ids)
    B = batch.BoardBatch(G)
    B.import_state(rb, rh)
    played, carried = None, 0
    for ply, budgets in enumerate(plan):
        rb, rh = B.export_state()
        bt = torch.tensor([budgets[0]] * (G // 2) + [budgets[1]] * (G // 2), dtype=torch.int32, device="cuda")
        action, policy, sum_n = mixed.search(rb, rh, played=played, budgets=bt)
        stats = [x.cpu().numpy() for x in mixed.carry_stats()]
        for k, ref in enumerate(refs):
            ref.sims = budgets[k]                               # this group's simulations at this ply: the existing path
            a, p, n = ref.search(rb, rh, played=played)
            rows = torch.tensor(group[k], device="cuda")
            assert torch.equal(action[rows], a[rows]) and torch.equal(sum_n[rows], n[rows]), (ply, k)
            assert torch.equal(_bits(policy)[rows], _bits(p)[rows]), (ply, k)
            for want, have in zip((x.cpu().numpy() for x in ref.carry_stats()), stats):
                assert np.array_equal(want[group[k]], have[group[k]]), (ply, k)
            for g in group[k]:
                _same_tree(mixed.export_tree(g), ref.export_tree(g), (ply, k, g))
        if ply:
            carried += int(stats[0].sum())
            assert not stats[2].any()
        played = action.clone()
        B.step(played)
    assert carried > 0 and B.illegal_count() == 0               # the second ply did start from kept trees
    for ts in [mixed] + refs:
        ts.close()
    B.close()


# ------------------------------------------------------------------------------------------ 4. rows
@pytest.mark.gpu
def test_dropped_out_games_cost_the_evaluator_no_rows():
    from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
    torch.manual_seed(0)
    net = InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16)
    G, sims, short = 64, 16, 2
    rb, rh = _roots(G, seed=31, games=8, skip=16)

    def run(s, budgets=None):
        ts = mcts.TreeSearch(G, s, net, seed=3, share_equal_leaves=False)
        assert ts.skip_unread_rows and not ts.share_equal_leaves
        ts.search(rb, rh, budgets=budgets)
        h = ts.leaf_histogram().cpu().numpy()
        out = (int(ts.evals_run.item()), h[:, 1] + h[:, 2], ts.evals_launched)
        ts.close()
        return out

    uniform, low = run(sims), run(short)
    for rows, needed, _ in (uniform, low):
        assert rows == int(needed.sum())
    bt = torch.tensor([short] * (G // 2) + [sims] * (G // 2), dtype=torch.int32, device="cuda")
    rows, needed, launched = run(sims, bt)
    expected = int(low[1][:G // 2].sum() + uniform[1][G // 2:].sum())
    print(f"rows evaluated: uniform {uniform[0]}, budget {short} {low[0]}, half and half {rows} (expected {expected}), "
          f"launched {launched}")
    assert rows == int(needed.sum()) == expected
    assert launched == uniform[2] and rows < uniform[0]         # the holes are launched, not evaluated


# ------------------------------------------------------------------------------------------ 5. the draw
@pytest.mark.gpu
def test_budget_draw_equals_the_mirror():
    L, check = _lib()
    n, seed = 4096, 0x5EED0123456789AB
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1 << 40, n)
    turns = rng.integers(1, 55, n)
    ids[7], turns[7] = ids[1000], turns[1000]                   # one key twice
    perm = rng.permutation(n)
    active = (rng.random(n) < 0.9).astype(np.int8)
    for p_full, order, act in ((0.25, np.arange(n), None), (0.25, perm, active), (0.6, perm, None), (0.0, perm, None),
                                (1.0, perm, None)):
        boards = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        boards[:, 33] = torch.from_numpy(turns[order].astype(np.uint8)).cuda()
        gid = torch.from_numpy(ids[order].astype(np.int64)).cuda()
        at = torch.from_numpy(act[order]).cuda() if act is not None else None
        budget = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        quiet = torch.full((n,), -9, dtype=torch.int8, device="cuda")
        full = torch.full((n,), -9, dtype=torch.int8, device="cuda")
        check(L.hive_search_draw_budgets(ctypes.c_uint64(seed), _p(gid), _p(boards), _p(at), n, 50, 10,
                                         mcts.full_threshold(p_full), _p(budget), _p(quiet), _p(full), _stream()))
        want = mcts.playout_cap_draw(seed, ids[order], turns[order], p_full)
        on = act[order] != 0 if act is not None else np.ones(n, dtype=bool)
        assert np.array_equal(full.cpu().numpy(), (want & on).astype(np.int8)), p_full
        assert np.array_equal(budget.cpu().numpy(), np.where(on, np.where(want, 50, 10), 0)), p_full
        assert np.array_equal(quiet.cpu().numpy(), (~want & on).astype(np.int8)), p_full
        if p_full in (0.0, 1.0):
            assert bool(want.all()) == (p_full == 1.0) and bool(want.any()) == (p_full == 1.0)
        else:
            assert 0 < want.sum() < n and want[np.flatnonzero(order == 7)[0]] == want[np.flatnonzero(order == 1000)[0]]
        # quiet and full are optional outputs
        b2 = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        check(L.hive_search_draw_budgets(ctypes.c_uint64(seed), _p(gid), _p(boards), _p(at), n, 50, 10,
                                         mcts.full_threshold(p_full), _p(b2), None, None, _stream()))
        assert torch.equal(b2, budget)


# (no GPU: the mirror alone)
def test_budget_draw_mirror_is_a_fair_coin_of_the_asked_weight():
    """100,000 draws of the mirror at p_full = 0.25: the full share lies within 5 binomial standard deviations,
    5 * sqrt(0.25 * 0.75 / 100000) = 0.0068, of 0.25; p_full 0 / 1 are never / always; the draw is a function of its key."""
    n = 100_000
    ids = np.arange(n, dtype=np.int64) // 50 + 7000
    turns = np.arange(n, dtype=np.int64) % 50 + 1
    full = mcts.playout_cap_draw(20260, ids, turns, 0.25)
    assert full.dtype == bool and full.shape == (n,)
    share = float(full.mean())
    print(f"full share {share:.5f}")
    assert abs(share - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / n) + 1e-12
    assert not mcts.playout_cap_draw(20260, ids, turns, 0.0).any()
    assert mcts.playout_cap_draw(20260, ids, turns, 1.0).all()
    perm = np.random.default_rng(0).permutation(n)
    assert np.array_equal(mcts.playout_cap_draw(20260, ids[perm], turns[perm], 0.25), full[perm])
    assert not np.array_equal(mcts.playout_cap_draw(20261, ids, turns, 0.25), full)
    # by turn and by game the share stays near 0.25: neither key is ignored (50 / 2000 groups, 6 sigma of a group's share)
    by_turn = full.reshape(-1, 50).mean(0)
    assert np.abs(by_turn - 0.25).max() < 6 * np.sqrt(0.25 * 0.75 / 2000)
    assert mcts.full_threshold(1.0) == 0xFFFFFFFF and mcts.full_threshold(0.0) == 0 and mcts.full_threshold(0.25) == 1 << 30
    with pytest.raises(ValueError):
        mcts.full_threshold(1.5)


# ------------------------------------------------------------------------------------------ 6. the arena's budgets
@pytest.mark.gpu
@pytest.mark.parametrize("games", [1, 63, 1000])
def test_arena_budget_equals_numpy(games):
    L, check = _lib()
    rng = np.random.default_rng(games)
    turn = rng.integers(1, 55, games).astype(np.uint8)
    aw = rng.integers(0, 2, games).astype(np.int8)
    boards = torch.zeros((games, 64), dtype=torch.uint8, device="cuda")
    boards[:, 33] = torch.from_numpy(turn).cuda()
    budget = torch.full((games + 1,), -9, dtype=torch.int32, device="cuda")
    check(L.hive_arena_budget_launch(_p(boards), _p(torch.from_numpy(aw).cuda()), games, 12, 3, _p(budget), _stream()))
    want = np.where((aw != 0) == (turn % 2 == 1), 12, 3)
    assert np.array_equal(budget[:games].cpu().numpy(), want) and budget[games].item() == -9
    if games > 1:
        assert set(want.tolist()) == {3, 12}
