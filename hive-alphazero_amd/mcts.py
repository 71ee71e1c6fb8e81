"""TreeSearch / SelfPlay: thousands of PUCT searches in lock step on one MI355X.

Python only sequences kernel launches; the tree (flat SoA node pool), selection, expansion and
backup are HIP kernels behind include/hive_search.h, leaf positions are expanded and encoded by
the env kernels (hive_leaf_launch), and the only MFMA work is the batched network forward
(alpha_net.InferenceNet) on [games x slots] leaves per simulation.
"""
import ctypes

import torch

from . import _lib
from ._lib import HIVE_MASK_WORDS, HWC, check, dtype_code, load, ptr as _p, stream_ptr
from .config import MAX_GAME_LENGTH
from .records import PlyLog, concat_packed, packed_games, rows_from_game, unpack_game
from .search_rules import *  # noqa: F401,F403  (the rules' numpy statements; every mcts.NAME of them keeps working)
from .search_rules import solver_answer, solver_edge_status, solver_holds, solver_node_status, solver_options  # noqa: F401


class _GumbelParams(ctypes.Structure):
    _fields_ = [("max_considered", ctypes.c_int32), ("c_visit", ctypes.c_float), ("c_scale", ctypes.c_float),
                ("sims", ctypes.c_int32)]


class _Params(ctypes.Structure):
    _fields_ = [("c_puct", ctypes.c_float), ("noise_eps", ctypes.c_float), ("dirichlet_alpha", ctypes.c_float),
                ("max_game_length", ctypes.c_int32), ("mode", ctypes.c_int32), ("virtual_loss", ctypes.c_float)]


class TreeSearch:
    """`games` independent searches of `sims` simulations each (HivePlayer.action, solo_play.py:110-165).

    evaluator(planes[B,12,12,56]) -> (p fp32 [B,1584] softmax, v fp32 [B])."""

    def __init__(self, games, sims, evaluator, device=None, slots=1, seed=0, plane_dtype=None,
                 c_puct=0.7, noise_eps=0.25, dirichlet_alpha=0.3, max_nodes=None, transpositions=True, mode=PUCT,
                 virtual_loss=None, max_game_length=None, skip_unread_rows=True, share_equal_leaves=True, reuse_store=0,
                 keep_tree=False, rolling=False, gumbel=None, gumbel_interior=False, solver=False):
        """mode = PUCT: woker/solo_play.py::HivePlayer; mode = UCT: alpha_zero/MCTS_chess.py::UCT_search (plain tree, no
        noise, no length cap; with one slot the virtual loss is 0 so that W sums exactly like the sequential reference).

        keep_tree: search(..., played=...) starts from the subtree under the move that was played since the previous
        search (hive_search_advance_roots) instead of from an empty tree; a tree that would leave fewer than
        sims + slots + 2 of the max_nodes (default then: 3 * sims + slots + 2) free is dropped (carry_stats).

        rolling: every game runs on its own clock (hive_search_set_rolling): restart() puts some games onto new roots while
        the others go on, run_rounds() advances every game by one round of `slots` simulations of its own search, and
        policy_where() answers the games that are done.  A game ends its search with the tree the lock-step search of its
        budget gives it, bit for bit.  Needs budgets (set_budgets); not with keep_tree, whose advance moves all trees at
        once.  search() / run_simulations() are the lock-step paths and stay as they are.

        gumbel = None (default) | True | {"m": 16, "c_visit": 50, "c_scale": 1.0}: the Gumbel root with sequential halving
        (hive_search_set_gumbel; the rule is stated in include/hive_search.h).  The root's simulations are spent by the
        halving schedule over the Gumbel-top-m edges instead of by PUCT with Dirichlet noise, the move is
        argmax(g + logit + sigma(q)) among the most visited edges and the policy is the improved policy
        softmax(logit + sigma(completed q)), dense over the legal moves, instead of the visit histogram.  Below the root the
        search is unchanged.  Works with budgets, quiet (g = 0: deterministic) and rolling; refused with slots > 1, UCT and
        keep_tree (gumbel_options).  c_visit / c_scale are the paper's values and have not been tuned here.
        set_gumbel_where(mask) restricts it to some games; the others are searched as without it, bit for bit.

        gumbel_interior = True (needs gumbel): the Gumbel rule also selects below the root
        (hive_search_set_gumbel_interior): at every deeper node the descent takes the edge whose visit share lags
        softmax(logit + sigma(completed q)) most, unvisited children completed by the node's mixed value, in place of PUCT.
        Deterministic, no c_puct; the root's schedule and answer are unchanged.  set_gumbel_interior(on, where) switches it
        and restricts it to some of the Gumbel games.

        solver = True: proven wins and losses below the root (hive_search_set_solver; the rule is stated in
        include/hive_search.h).  A finished game with a winner proves its node, the proof travels up the path of the
        simulation that found it, a proven node ends later descents without a network row, moves proven to lose are left out
        of PUCT and of the answer, and a proven root answers with the fastest win or the longest resistance.  The policy row
        and sum_n stay the visit distribution.  Draws and the length cap prove nothing.  Works with slots > 1, budgets,
        rolling and keep_tree; refused in UCT mode and together with gumbel (solver_options).  set_solver(on, where)
        switches it and restricts it to some games; the others are searched as without it, bit for bit."""
        gumbel = gumbel_options(gumbel, slots, mode, keep_tree)
        solver = solver_options(solver, mode, gumbel)
        gumbel_interior = gumbel_interior_options(gumbel_interior, gumbel)
        if rolling and keep_tree:
            raise ValueError("TreeSearch: rolling cannot keep trees (hive_search_advance_roots moves every tree at once)")
        L = load()
        if L.hive_device_count() <= 0 or not torch.cuda.is_available():
            raise _lib.HiveError(-2, "no HIP device visible: hive_alphazero_amd has no CPU path")
        if plane_dtype is None:      # the evaluator's own input type (the plane values 0 / 1 / turn are exact in all three)
            plane_dtype = getattr(evaluator, "dtype", torch.bfloat16)
            if plane_dtype not in (torch.float32, torch.float16, torch.bfloat16):
                plane_dtype = torch.bfloat16
        self.L = L
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.games, self.sims, self.slots, self.evaluator = games, sims, slots, evaluator
        self.keep_tree = bool(keep_tree)
        self.max_nodes = max_nodes or ((3 * sims if self.keep_tree else sims) + slots + 2)
        self._h = ctypes.c_void_p()
        check(L.hive_search_create(games, self.max_nodes, slots, self.device.index, seed, ctypes.byref(self._h)))
        if self.keep_tree:
            check(L.hive_search_set_carry_room(self._h, sims + slots + 2))
            self._unrelated = torch.full((games,), -3, dtype=torch.int32, device=self.device)
        self.rolling = bool(rolling)
        if self.rolling:
            check(L.hive_search_set_rolling(self._h, 1))
            self.done = torch.zeros((games,), dtype=torch.int8, device=self.device)
            self.root_feat = torch.zeros((games, 144), dtype=torch.int64, device=self.device)
            self._clock = torch.zeros((games,), dtype=torch.int32, device=self.device)
        self.mode = mode
        if mode == UCT:
            noise_eps, transpositions = 0.0, False
            if virtual_loss is None:
                virtual_loss = 0.0 if slots == 1 else 1.0
            if max_game_length is None:
                max_game_length = 250
        prm = _Params(c_puct, noise_eps, dirichlet_alpha, MAX_GAME_LENGTH if max_game_length is None else max_game_length,
                      mode, 1.0 if virtual_loss is None else virtual_loss)
        check(L.hive_search_set_params(self._h, ctypes.byref(prm)))
        # the reference's tree is a dict keyed by state_key: positions reached by two move orders share one entry
        check(L.hive_search_set_transpositions(self._h, 1 if transpositions else 0))
        self.gumbel = self._gumbel_where = self._gumbel_sims = None
        if gumbel is not None:
            self.set_gumbel(gumbel)
        self.gumbel_interior, self._gumbel_interior_where = False, None
        if gumbel_interior:
            self.set_gumbel_interior(True)
        self.solver, self._solver_where = False, None
        if solver:
            self.set_solver(True)
        n = games * slots
        dev = self.device
        self.plane_dtype = plane_dtype
        self.leaf_boards = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        self.leaf_hist = torch.zeros((n, 384), dtype=torch.uint8, device=dev)
        self.leaf_mask = torch.zeros((n, HIVE_MASK_WORDS), dtype=torch.int32, device=dev)
        self.leaf_count = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.leaf_over = torch.zeros((n,), dtype=torch.int8, device=dev)
        self.leaf_winner = torch.zeros((n,), dtype=torch.int8, device=dev)
        self.planes = torch.zeros((n, 12, 12, 56), dtype=plane_dtype, device=dev)
        self.workspace = torch.zeros((n * 144,), dtype=torch.int64, device=dev)
        self.policy = torch.zeros((games, 1584), dtype=torch.float32, device=dev)
        self.action = torch.zeros((games,), dtype=torch.int32, device=dev)
        self.sum_n = torch.zeros((games,), dtype=torch.int32, device=dev)
        self.root_planes = None
        self._budgets = self._quiet = None      # per-game budgets of the current search (the handle keeps their addresses)
        # rows of the leaf batch whose prediction the backup never reads (finished games, length cap, collisions, idle
        # trees: the reference does not call its model for them either, solo_play.py:169-197) are skipped by an evaluator
        # that can (InferenceNet: its tower kernels take the flags); evals_run counts the rows that were evaluated
        self.skip_unread_rows = bool(skip_unread_rows) and bool(getattr(evaluator, "accepts_need", False))
        self.leaf_need = torch.ones((n,), dtype=torch.int8, device=dev)
        self.evals_run = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.evals_launched = 0
        # equal leaves of one batch (same board record and history = same planes) are evaluated once: lock-step games from
        # the opening ask about the same few positions (hive_leaf_dedup_launch; batches of up to 4096 rows)
        self.share_equal_leaves = (self.skip_unread_rows and bool(share_equal_leaves) and n <= 4096
                                   and bool(getattr(evaluator, "accepts_rep", False)))
        if self.skip_unread_rows and share_equal_leaves and n > 4096 and getattr(evaluator, "accepts_rep", False):
            import warnings
            warnings.warn(f"TreeSearch: leaf batches of {n} rows exceed hive_leaf_dedup_launch's 4096-row table; equal leaves "
                          "are evaluated separately (share_equal_leaves off)")
        self.leaf_rep = torch.arange(n, dtype=torch.int32, device=dev)
        self.leaf_keys = torch.zeros((n,), dtype=torch.int64, device=dev)
        # evaluations kept ACROSS searches (hive_leaf_store_*, include/hive_abi.h): the reference empties its tree on every
        # move (solo_play.py:103-112) and evaluates the subtree under the played move again; reuse_store = entries (0 = off,
        # the default).  Needs the equal-leaf keys; the served rows are counted apart from the evaluated ones (rows_served).
        self._store = None
        self._store_version = getattr(evaluator, "weights_version", 0)
        if reuse_store and self.share_equal_leaves and getattr(evaluator, "batch_independent_bits", False):
            self._store = ctypes.c_void_p()
            check(L.hive_leaf_store_create(self.device.index, int(reuse_store), ctypes.byref(self._store)))
            self.leaf_hit = torch.full((n,), -1, dtype=torch.int32, device=dev)

    def close(self):
        if getattr(self, "_h", None):
            self.L.hive_search_destroy(self._h)
            self._h = None
        if getattr(self, "_store", None):
            self.L.hive_leaf_store_destroy(self._store)
            self._store = None

    def rows_served(self):
        """(rows answered from the store, rows inserted into it) since it was created or cleared."""
        if self._store is None:
            return 0, 0
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.L.hive_leaf_store_stats(self._store, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        s = stream_ptr(self.device)
        check(self.L.hive_search_set_stream(self._h, s))
        return s

    def _evaluate(self, k, n, s):
        """The network's (p, v) for the n = k * games leaves of this round of simulations (rows the backup never reads,
        and duplicates of an evaluated row, are switched off for an evaluator that takes the flags), as the evaluator returns
        them: _round makes them the backup's fp32 rows and, with a store, inserts them into it (hive_leaf_store_update;
        the lookup happens here, before the network runs)."""
        L = self.L
        if self.skip_unread_rows:
            check(L.hive_search_leaf_need(self._h, k, _p(self.leaf_boards), _p(self.leaf_over), _p(self.leaf_need),
                                          _p(self.evals_run)))
            if self.share_equal_leaves:
                check(L.hive_leaf_dedup_launch(_p(self.leaf_boards), _p(self.leaf_hist), n, _p(self.leaf_need),
                                               _p(self.leaf_rep), _p(self.leaf_keys), _p(self.evals_run), s))
                if self._store is not None:
                    if getattr(self.evaluator, "weights_version", 0) != self._store_version:      # new weights: old answers are void
                        check(L.hive_leaf_store_clear(self._store, s))
                        self._store_version = getattr(self.evaluator, "weights_version", 0)
                    check(L.hive_leaf_store_lookup(self._store, _p(self.leaf_boards), _p(self.leaf_hist), n, _p(self.leaf_keys),
                                                   _p(self.leaf_need), _p(self.leaf_hit), _p(self.evals_run), s))
                p, v = self.evaluator(self.planes[:n], need=self.leaf_need[:n], rep=self.leaf_rep[:n])
            else:
                p, v = self.evaluator(self.planes[:n], need=self.leaf_need[:n])
        else:
            p, v = self.evaluator(self.planes[:n])
        self.evals_launched += n
        return p, v

    def _round(self, k, between=None):
        """One round of simulations, the only place that issues one: select for slots 0 .. k-1, the leaf launch over the
        n = k * games rows, between() (a caller's read of the leaf buffers before the network runs), the evaluation and the
        backup of slots 0 .. k-1.  The handle's stream is the caller's (_stream())."""
        L, G, s = self.L, self.games, stream_ptr(self.device)
        for sl in range(k):
            check(L.hive_search_select(self._h, sl, _p(self.leaf_boards[sl * G:]), _p(self.leaf_hist[sl * G:])))
        n = k * G
        check(L.hive_leaf_launch(_p(self.leaf_boards), _p(self.leaf_hist), n, _p(self.planes), dtype_code(self.plane_dtype),
                                 HWC, _p(self.workspace), _p(self.leaf_mask), _p(self.leaf_count),
                                 _p(self.leaf_over), _p(self.leaf_winner), s))
        if between is not None:
            between()
        p, v = self._evaluate(k, n, s)
        p = p.float().contiguous()
        v = v.float().contiguous().view(-1)
        if self._store is not None:      # the round's answers join the kept evaluations (fp32 rows, like the backup's)
            check(L.hive_leaf_store_update(self._store, _p(self.leaf_boards), _p(self.leaf_hist), n, _p(self.leaf_keys),
                                           _p(self.leaf_need), _p(self.leaf_rep), _p(self.leaf_hit), _p(p), _p(v), s))
        for sl in range(k):
            o = sl * G
            check(L.hive_search_backup(self._h, sl, _p(self.leaf_boards[o:]), _p(self.leaf_hist[o:]),
                                       _p(self.leaf_mask[o:]), _p(self.leaf_over[o:]), _p(self.leaf_winner[o:]),
                                       _p(p[o:]), _p(v[o:])))

    def _games_mask(self, x, dtype=torch.int8):
        """x as a contiguous device tensor of `dtype` with one entry per game."""
        x = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
        assert x.numel() == self.games
        return x

    def _read(self, fn, *tail, count=1, dtype=torch.int32, alloc=torch.zeros):
        """One of the library's per-game readers: `count` fresh [games, *tail] tensors filled by fn(handle, out, ...) on the
        current stream -> the tensor, or the list of them."""
        out = [alloc((self.games,) + tail, dtype=dtype, device=self.device) for _ in range(count)]
        self._stream()
        check(fn(self._h, *[_p(t) for t in out]))
        return out[0] if count == 1 else out

    def advance_roots(self, root_boards, root_hist, active=None, played=None):
        """keep_tree only: the roots of the next search, each tree cut down to the subtree under `played`
        (hive_search_advance_roots); search() = advance_roots() + run_simulations()."""
        if not self.keep_tree:
            raise ValueError("TreeSearch.advance_roots needs keep_tree=True")
        self._stream()
        if played is None:
            played = self._unrelated
        else:
            played = torch.as_tensor(played, dtype=torch.int32, device=self.device).contiguous()
            assert played.numel() == self.games
        check(self.L.hive_search_advance_roots(self._h, _p(played), _p(root_boards), _p(root_hist), _p(active)))

    def set_budgets(self, budgets=None, quiet=None):
        """Per-game simulation budgets of the searches from now on (hive_search_set_budgets): budgets int32[games], quiet
        int8[games] (1 = no root noise for that game), device tensors that this object keeps alive; None, None = off.
        `sims` stays the number of simulations the batch runs; a budget given on the host is checked against it (a device
        tensor is taken as it is: a budget above `sims` then simply ends at `sims`)."""
        if budgets is None:
            if quiet is not None:
                raise ValueError("TreeSearch: quiet needs budgets")
        else:
            if not (isinstance(budgets, torch.Tensor) and budgets.is_cuda):
                host = torch.as_tensor(budgets).reshape(-1)
                if host.numel() and int(host.max()) > self.sims:
                    raise ValueError(f"TreeSearch: a budget of {int(host.max())} simulations exceeds sims={self.sims}")
            budgets = self._games_mask(budgets, torch.int32)
            if quiet is not None:
                quiet = self._games_mask(quiet)
        self._budgets, self._quiet = budgets, quiet
        check(self.L.hive_search_set_budgets(self._h, _p(budgets), _p(quiet)))

    def set_gumbel(self, gumbel=True, where=None):
        """Switch the Gumbel root on (True or the option dict of __init__), for the games with where[g] != 0 (int8 / bool
        [games]; None = every game), or off (None / False): hive_search_set_gumbel."""
        opt = gumbel_options(gumbel, self.slots, self.mode, self.keep_tree)
        if opt is not None:
            solver_options(getattr(self, "solver", False), self.mode, opt)
        if opt is None:
            check(self.L.hive_search_set_gumbel(self._h, None, None))
            self.gumbel = self._gumbel_where = self._gumbel_sims = None
            return
        if where is not None:
            where = self._games_mask(where)
        prm = _GumbelParams(opt["m"], opt["c_visit"], opt["c_scale"], int(self.sims))
        check(self.L.hive_search_set_gumbel(self._h, ctypes.byref(prm), _p(where)))
        # (the handle keeps the address of `where`: this object keeps the tensor)
        self.gumbel, self._gumbel_where, self._gumbel_sims = opt, where, int(self.sims)

    def set_gumbel_where(self, mask):
        """The games the Gumbel root applies to from now on: int8 / bool [games], None = every game."""
        if self.gumbel is None:
            raise ValueError("TreeSearch.set_gumbel_where: the Gumbel root is off (gumbel=... / set_gumbel)")
        self.set_gumbel(self.gumbel, mask)

    def set_gumbel_interior(self, on=True, where=None):
        """The Gumbel rule below the root on or off, for the Gumbel games with where[g] != 0 (int8 / bool [games]; None =
        every Gumbel game): hive_search_set_gumbel_interior.  It acts on Gumbel games only and survives set_gumbel(None) /
        set_gumbel(...): switching the Gumbel root off and on leaves it as it was."""
        where = self._games_mask(where) if on and where is not None else None
        check(self.L.hive_search_set_gumbel_interior(self._h, 1 if on else 0, _p(where)))
        # (the handle keeps the address of `where`: this object keeps the tensor)
        self.gumbel_interior, self._gumbel_interior_where = bool(on), where

    def set_solver(self, on=True, where=None):
        """Proven wins and losses on or off, for the games with where[g] != 0 (int8 / bool [games]; None = every game):
        hive_search_set_solver."""
        on = solver_options(bool(on), self.mode, self.gumbel)
        where = self._games_mask(where) if on and where is not None else None
        self._stream()
        check(self.L.hive_search_set_solver(self._h, 1 if on else 0, _p(where)))
        # (the handle keeps the address of `where`: this object keeps the tensor)
        self.solver, self._solver_where = on, where

    def node_status(self, game):
        """(node int8[n], edge int8[n,256]): the statuses of game `game`'s tree in export_tree's node and edge order
        (hive_search_node_status); of a node's edge row only the first nedge entries are meaningful."""
        node = torch.zeros((self.max_nodes,), dtype=torch.int8, device=self.device)
        edge = torch.zeros((self.max_nodes, 256), dtype=torch.int8, device=self.device)
        count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._stream()
        check(self.L.hive_search_node_status(self._h, int(game), _p(node), _p(edge)))
        check(self.L.hive_search_export_tree(self._h, int(game), _p(count), *([None] * 11)))
        n = int(count.item())
        return node[:n].cpu().numpy(), edge[:n].cpu().numpy()

    def root_status(self):
        """int8[games]: the stored status of every root (hive_search_root_status)."""
        return self._read(self.L.hive_search_root_status, dtype=torch.int8)

    def solver_stats(self):
        """int32[games,4] since create: descents ended at a proven node, nodes that became proven wins, proven losses,
        answers taken from a proof (hive_search_solver_stats)."""
        return self._read(self.L.hive_search_solver_stats, 4)

    def node_values(self, game):
        """float32[n]: the value every node of game `game`'s tree was created with, in export_tree's node order
        (hive_search_node_values)."""
        out = torch.zeros((self.max_nodes,), dtype=torch.float32, device=self.device)
        count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._stream()
        check(self.L.hive_search_node_values(self._h, int(game), _p(out)))
        check(self.L.hive_search_export_tree(self._h, int(game), _p(count), *([None] * 11)))
        return out[:int(count.item())].cpu().numpy()

    def root_gumbel(self):
        """(g, logit, completed q, improved policy) fp32[games,256] of the roots as they stand, in edge order (ascending
        action id; zeros past the last edge): hive_search_root_gumbel."""
        return self._read(self.L.hive_search_root_gumbel, 256, count=4, dtype=torch.float32)

    def gumbel_fallbacks(self):
        """int32[games]: root selections since create that found no edge at the scheduled visit count."""
        return self._read(self.L.hive_search_gumbel_fallbacks)

    def search(self, root_boards, root_hist, active=None, selfplay=False, keep_root_planes=False, played=None, budgets=None,
               quiet=None):
        """-> (action int32[games] (-1 pass, -2 inactive/terminal root), policy fp32[games,1584], sum_n int32[games])

        played (keep_tree only): int32[games], the action that led from the previous search's root to root_boards
        (-1 pass, -3 unrelated position; None = all -3).
        budgets / quiet: set_budgets for this search -- game g takes part in the first budgets[g] of the `sims` simulations
        and ends with the tree TreeSearch(sims=budgets[g]) would have given it; None = every game gets all of them."""
        L, G = self.L, self.games
        s = self._stream()
        if budgets is not None or self._budgets is not None:
            self.set_budgets(budgets, quiet)
        elif quiet is not None:
            raise ValueError("TreeSearch: quiet needs budgets")
        if self.keep_tree:
            self.advance_roots(root_boards, root_hist, active, played)
            if keep_root_planes:
                # a carried root is never a leaf, so the records' feature words come from an encode of the roots themselves
                # (the kernel code hive_leaf_launch runs on a fresh root; the leaf launches then reuse both buffers)
                check(L.hive_encode_launch(_p(root_boards), _p(root_hist), G, _p(self.planes), dtype_code(self.plane_dtype),
                                           HWC, _p(self.workspace), s))
                self.root_planes = self.workspace[:G * 144].clone()
                keep_root_planes = False
        else:
            if played is not None:
                raise ValueError("TreeSearch.search: played needs keep_tree=True")
            check(L.hive_search_set_roots(self._h, _p(root_boards), _p(root_hist), _p(active)))
        return self.run_simulations(selfplay, keep_root_planes)

    def run_simulations(self, selfplay=False, keep_root_planes=False):
        """`sims` simulations from the roots as they stand, then the policy: the second half of search()."""
        L, G = self.L, self.games
        self._stream()
        if self.gumbel is not None and self._gumbel_sims != self.sims:      # the schedule's length follows `sims`
            self.set_gumbel(self.gumbel, self._gumbel_where)

        def keep_roots():      # the opening round's leaves are the roots
            self.root_planes = self.workspace[:G * 144].clone()
        done = 0
        while done < self.sims:
            k = min(self.slots, self.sims - done) if done else 1      # the first simulation only opens the root
            self._round(k, keep_roots if keep_root_planes and not done else None)
            done += k
        check(L.hive_search_policy(self._h, _p(self.policy), _p(self.action), _p(self.sum_n), 1 if selfplay else 0))
        return self.action, self.policy, self.sum_n

    # ---- rolling: every game on its own clock
    def _need_rolling(self):
        if not self.rolling:
            raise ValueError("TreeSearch: this call needs rolling=True")

    def restart(self, which, root_boards, root_hist, active=None):
        """The games with which[g] != 0 (int8 / bool [games]) start a new search from root_boards[g] / root_hist[g], clock 0;
        every other game keeps its tree and its clock (hive_search_restart)."""
        self._need_rolling()
        which = self._games_mask(which)
        self._stream()
        check(self.L.hive_search_restart(self._h, _p(which), _p(root_boards), _p(root_hist), _p(active)))

    def run_rounds(self, rounds, keep_root_planes=False):
        """`rounds` rounds: every game that still has budget runs up to `slots` simulations of its own search per round (the
        root-opening one alone).  -> done int8[games] after the last round (a buffer of this object).
        keep_root_planes: root_feat int64[games,144] takes the packed feature words of the roots opened in these rounds --
        at clock 0 a game's slot-0 leaf is its root.  Restarts happen between calls, so only the first round can open one."""
        self._need_rolling()
        L, G = self.L, self.games
        self._stream()

        def keep_roots():
            torch.where((self._clock == 0).view(G, 1), self.workspace[:G * 144].view(G, 144), self.root_feat,
                        out=self.root_feat)
        for r in range(rounds):
            opening = keep_root_planes and r == 0
            if opening:
                check(L.hive_search_clocks(self._h, _p(self._clock)))
            self._round(self.slots, keep_roots if opening else None)
            check(L.hive_search_round_end(self._h, self.slots, _p(self.done)))
        return self.done

    def policy_where(self, which, selfplay=False):
        """search()'s answer for the games with which[g] != 0; every other game gets a zero row, action -2 and sum 0
        (hive_search_policy_where).  -> (action, policy, sum_n), buffers of this object."""
        which = self._games_mask(which)
        self._stream()
        check(self.L.hive_search_policy_where(self._h, _p(which), _p(self.policy), _p(self.action), _p(self.sum_n),
                                              1 if selfplay else 0))
        return self.action, self.policy, self.sum_n

    def clocks(self):
        """int32[games]: the simulations every game's current search has run (hive_search_clocks)."""
        self._need_rolling()
        return self._read(self.L.hive_search_clocks)

    def set_game_ids(self, ids):
        """Global game index per tree (int64[games]): the only per-game key of the noise streams (hive_search.h)."""
        ids = self._games_mask(ids, torch.int64)
        self._stream()
        check(self.L.hive_search_set_game_ids(self._h, _p(ids)))

    def root_stats(self):
        """(visits, total_value, priors) fp32[games,1584]: the root's UCTNode arrays (MCTS_chess.py:33-35)."""
        return self._read(self.L.hive_search_root_stats, 1584, count=3, dtype=torch.float32, alloc=torch.empty)

    def leaf_histogram(self):
        """int32[games,8] leaves by kind since create (LEAF_KINDS)."""
        return self._read(self.L.hive_search_leaf_histogram, 8)

    def node_counts(self):
        return self._read(self.L.hive_search_node_counts)

    def carry_stats(self):
        """(kept_nodes, carried_visits, refused) int32[games]: nodes / root visits the last search started with (0 = fresh
        tree) and the trees dropped for lack of room in the pool since create (hive_search_carry_stats)."""
        return self._read(self.L.hive_search_carry_stats, count=3)

    def export_tree(self, g):
        """Game g's tree as numpy arrays (hive_search_export_tree), cut to its n nodes: {"n", "board" uint8[n,64], "hist"
        uint8[n,384], "nedge", "sum_n", "term", "tv" [n], "act", "p", "n_visits", "w", "child" [n,256]}; of a node's
        edge rows only the first nedge entries are meaningful."""
        M, dev = self.max_nodes, self.device
        spec = [("board", (M, 64), torch.uint8), ("hist", (M, 384), torch.uint8), ("nedge", (M,), torch.int32),
                ("sum_n", (M,), torch.int32), ("term", (M,), torch.int8), ("tv", (M,), torch.float32),
                ("act", (M, 256), torch.int16), ("p", (M, 256), torch.float32), ("n_visits", (M, 256), torch.int32),
                ("w", (M, 256), torch.float32), ("child", (M, 256), torch.int32)]
        n = torch.zeros((1,), dtype=torch.int32, device=dev)
        bufs = [torch.zeros(shape, dtype=dt, device=dev) for _, shape, dt in spec]
        self._stream()
        check(self.L.hive_search_export_tree(self._h, int(g), _p(n), *[_p(b) for b in bufs]))
        count = int(n.item())
        out = {name: b[:count].cpu().numpy() for (name, _, _), b in zip(spec, bufs)}
        out["n"] = count
        return out

    def transposition_hits(self):
        """int32[games]: descents that continued through a node first reached by another move order."""
        return self._read(self.L.hive_search_transposition_hits)


class ArenaSearch(TreeSearch):
    """TreeSearch whose games are searched by TWO networks (woker/evaluation.py: one HivePlayer per side, each with its own
    model): the search of game g is the thinking of the side to move at its root, so all its leaves go to network A iff
    a_white[g] == (root turn is odd), else to network B.  a_white = device int8[games], read at every search (the caller
    may rewrite it in place between searches).  Both networks see the same leaf batch with their own row flags
    (hive_arena_split_launch): a tower costs what its own rows cost; equal leaves are shared within a network, never
    across.  hive_arena_join_launch merges the two predictions for the backup.

    An evaluator without `accepts_need` (a stub, the library path) gets the whole batch.  `rows_evaluated()` = the rows
    each network evaluated; `evals_run` is their sum.  reuse_store is refused: the store's key does not hold the network;
    keep_tree for the same reason (a kept tree holds the other network's evaluations).

    gumbel_a / gumbel_b (None | True | dict, as TreeSearch's gumbel): the side searches with the Gumbel root.  At every search
    game g is a Gumbel game iff the owner of its search -- the rule above -- has the option; the other side's games are
    searched as without it, bit for bit.  One handle holds one parameter set: two dicts must be equal.
    gumbel_interior_a / gumbel_interior_b: that side's Gumbel searches also select below the root by the Gumbel rule
    (TreeSearch, gumbel_interior); a side with it must have gumbel_*.  gumbel_a=True, gumbel_b=True, gumbel_interior_a=True
    is full Gumbel against root-only Gumbel on one handle.
    solver_a / solver_b: that side searches with proven wins and losses (TreeSearch, solver), by the same ownership rule;
    not on a handle where either side has the Gumbel root."""

    def __init__(self, games, sims, evaluator_a, evaluator_b, a_white, device=None, slots=1, seed=0, plane_dtype=None,
                 gumbel_a=None, gumbel_b=None, gumbel_interior_a=False, gumbel_interior_b=False, solver_a=False,
                 solver_b=False, **options):
        if options.get("reuse_store"):
            raise ValueError("ArenaSearch: reuse_store keeps evaluations by position alone, not by network")
        if options.get("keep_tree"):
            raise ValueError("ArenaSearch: keep_tree would hand one network's evaluations to the other, whose ply is next")
        if options.get("rolling"):
            raise ValueError("ArenaSearch: rolling is not built for the arena (both sides' searches run in lock step)")
        if options.get("gumbel"):
            raise ValueError("ArenaSearch: give the Gumbel root per side, gumbel_a / gumbel_b")
        if options.get("gumbel_interior"):
            raise ValueError("ArenaSearch: give the interior rule per side, gumbel_interior_a / gumbel_interior_b")
        if options.get("solver"):
            raise ValueError("ArenaSearch: give proven results per side, solver_a / solver_b")
        sides = [gumbel_options(x, slots, options.get("mode", PUCT)) for x in (gumbel_a, gumbel_b)]
        if sides[0] is not None and sides[1] is not None and sides[0] != sides[1]:
            raise ValueError("ArenaSearch: one handle holds one Gumbel parameter set; gumbel_a and gumbel_b differ")
        interior = (gumbel_interior_options(gumbel_interior_a, sides[0]), gumbel_interior_options(gumbel_interior_b, sides[1]))
        # (one handle: a side with proven results cannot meet a side with the Gumbel root)
        solver = tuple(solver_options(x, options.get("mode", PUCT), sides[0] or sides[1]) for x in (solver_a, solver_b))
        super().__init__(games, sims, evaluator_a, device, slots, seed, plane_dtype,
                         **dict(options, gumbel=sides[0] or sides[1], solver=solver[0] or solver[1]))
        self._solver_sides = solver
        if solver[0] != solver[1]:                              # one side only: rewritten in place from the ownership rule
            self.set_solver(True, torch.zeros((games,), dtype=torch.int8, device=self.device))
        self._gumbel_sides = (sides[0] is not None, sides[1] is not None)
        if self._gumbel_sides[0] != self._gumbel_sides[1]:      # one side only: the mask is rewritten in place at every search
            self.set_gumbel_where(torch.zeros((games,), dtype=torch.int8, device=self.device))
        self._interior_sides = interior
        if interior[0] != interior[1]:                          # likewise: rewritten in place from the ownership rule
            self.set_gumbel_interior(True, torch.zeros((games,), dtype=torch.int8, device=self.device))
        elif interior[0]:
            self.set_gumbel_interior(True)
        self.evaluator_a, self.evaluator_b = evaluator_a, evaluator_b
        assert a_white.dtype == torch.int8 and a_white.numel() == games and a_white.is_cuda and a_white.is_contiguous()
        self.a_white = a_white
        n, dev = games * slots, self.device
        skip, share = bool(options.get("skip_unread_rows", True)), bool(options.get("share_equal_leaves", True))
        self._nets = []
        for k, e in enumerate((evaluator_a, evaluator_b)):
            flags = skip and bool(getattr(e, "accepts_need", False))
            self._nets.append({
                "evaluator": e, "flags": flags,
                "share": flags and share and n <= 4096 and bool(getattr(e, "accepts_rep", False)),
                "need": torch.ones((n,), dtype=torch.int8, device=dev),
                "rep": torch.arange(n, dtype=torch.int32, device=dev),
                "keys": torch.zeros((n,), dtype=torch.int64, device=dev)})
        self.rows = torch.zeros((2,), dtype=torch.int64, device=dev)        # rows evaluated by A, by B
        self._roots = None

    def rows_evaluated(self):
        """(rows network A evaluated, rows network B evaluated) since create."""
        a, b = self.rows.cpu().tolist()
        return int(a), int(b)

    def search(self, root_boards, root_hist, active=None, selfplay=False, keep_root_planes=False, budgets=None, quiet=None):
        self._roots = root_boards
        if self._gumbel_where is not None or self._gumbel_interior_where is not None or self._solver_where is not None:
            # the owner of the search of game g (hive_arena_budget_launch's rule): A iff a_white[g] == (root turn is odd)
            a_owns = (self.a_white != 0) == ((root_boards[:, 33] & 1) != 0)
            if self._gumbel_where is not None:
                self._gumbel_where.copy_(a_owns if self._gumbel_sides[0] else ~a_owns)
            if self._gumbel_interior_where is not None:
                self._gumbel_interior_where.copy_(a_owns if self._interior_sides[0] else ~a_owns)
            if self._solver_where is not None:
                self._solver_where.copy_(a_owns if self._solver_sides[0] else ~a_owns)
        out = super().search(root_boards, root_hist, active, selfplay, keep_root_planes, budgets=budgets, quiet=quiet)
        torch.sum(self.rows, 0, keepdim=True, out=self.evals_run)
        return out

    def _evaluate(self, k, n, s):
        L, A, B = self.L, self._nets[0], self._nets[1]
        check(L.hive_search_leaf_need(self._h, k, _p(self.leaf_boards), _p(self.leaf_over), _p(self.leaf_need), None))
        counters = [ctypes.c_void_p(self.rows.data_ptr() + 8 * i) if net["flags"] else None for i, net in enumerate(self._nets)]
        check(L.hive_arena_split_launch(_p(self._roots), _p(self.a_white), _p(self.leaf_need), self.games, k,
                                        _p(A["need"]), _p(B["need"]), counters[0], counters[1], s))
        for net, counter in zip(self._nets, counters):
            if net["share"]:
                check(L.hive_leaf_dedup_launch(_p(self.leaf_boards), _p(self.leaf_hist), n, _p(net["need"]), _p(net["rep"]),
                                               _p(net["keys"]), counter, s))
        out = []
        for i, net in enumerate(self._nets):
            if net["share"]:
                p, v = net["evaluator"](self.planes[:n], need=net["need"][:n], rep=net["rep"][:n])
            elif net["flags"]:
                p, v = net["evaluator"](self.planes[:n], need=net["need"][:n])
            else:
                p, v = net["evaluator"](self.planes[:n])
                self.rows[i] += n
            # (hive_arena_join_launch takes fp32 rows, so both predictions are converted here; _round's conversion of the
            # joined pair is then a no-op)
            out.append((p.float().contiguous(), v.float().contiguous().view(-1)))
        (p, v), (pb, vb) = out
        if p.data_ptr() == pb.data_ptr():        # (an evaluator that hands out one static buffer, called twice)
            raise _lib.HiveError(-1, "ArenaSearch: the two evaluators returned the same output buffer")
        check(L.hive_arena_join_launch(_p(self._roots), _p(self.a_white), self.games, k, _p(p), _p(v), _p(pb), _p(vb), s))
        self.evals_launched += n
        return p, v


def _override(action, forced):
    """play_ply's `forced` (SelfPlay, Arena): entries >= -1 replace the engine's move of a slot that moves; -2, or
    forced = None, keep it."""
    if forced is None:
        return action
    forced = torch.as_tensor(forced, dtype=torch.int32, device=action.device)
    return torch.where((forced >= -1) & (action != -2), forced, action)


class SelfPlay:
    """`games` self-play games advanced ply by ply (woker/self_play.py:116-193 for every game at once):
    search -> move selection (self-play noise on turns 1..6) -> env step; finished games (queen
    surrounded or turn >= 55) are scored and their slot takes the next game id.  Records per ply: the packed
    56-bit-per-cell features of the position, the visit policy and the mover; the value is filled
    in when the game ends (draw or length cap => -1 for both sides, self_play.py:188-189).

    Game ids: `game_ids` is an iterator of GLOBAL game indices this engine may play (default 0, 1, 2, ...; a
    multi-GPU run hands every rank its own shard, dist.game_id_stream).  All randomness of game i -- root noise,
    move resampling -- is keyed on (seed, i, turn, simulation), so its record does not depend on the slot, batch
    size, process or GPU it ran on.  When the iterator is exhausted a finishing slot goes idle.

    The host side of the records is records.PlyLog: it keeps the per-ply host copies and cuts the games that end on a
    ply into one packed batch (records.pack_games' arrays: no per-row Python objects, sparse policies).  This class owns
    only the GPU side of that: the copy stream, the pinned staging buffers and their events.  `packed_records` selects the
    container the caller drains: True keeps the batches (`drain_finished_packed()`; what SelfPlayWorker's children send
    to the parent), False expands every game of a batch into `finished_games` as (value_white, plies, game_id)
    (`drain_finished()`; per-row tuples with dense policies, for a few hundred games).  More than `max_finished_kept`
    undrained games are dropped and counted (`dropped_games`, one warning).

    playout_cap = {"full": 50, "fast": 10, "p_full": 0.25, "quiet_fast": True} (default None: every ply gets `sims`
    simulations): playout-cap randomisation.  Every ply of every game is drawn full (probability p_full) or fast by
    hive_search_draw_budgets from (seed, game id, turn) and searched with that many of the `sims` = max(full, fast)
    simulations; a fast ply is searched without root noise (quiet_fast, default True).  Move selection is unchanged.  A fast
    ply stays a row of its game, marked 0 in the packed batch's `full` key (records.FULL_KEY): datasets and the replay
    window take the rows marked 1.  With keep_records this needs packed_records=True -- the 6-tuples of the row-wise
    route have no room for the flag.  p_full = 1 with full == fast == sims plays the plain engine's games bit for bit.

    rolling = True or {"quantum": q} (default None: lock step): every game moves when its OWN search is done.  play_ply() is
    then one turn-over: q rounds of the rolling search (TreeSearch.run_rounds), the games whose search is complete move and
    log their ply, and each of them -- and every slot that took a new game -- draws its next budget and starts its next
    search in the following round while its neighbours go on with theirs.  With a playout cap no round then waits for the
    full plies: q defaults to the rounds of the shorter search, 1 + ceil((min(full, fast) - 1) / slots).  `plies` counts
    turn-overs in this mode, not plies of a game; the log entry of a turn-over holds the games that moved in it.  Every
    game's record is, bit for bit, the record the lock-step engine gives that game id (without playout_cap: the plain
    engine's).  Not with search_options keep_tree (ValueError).

    search_options = {"gumbel": True | {"m", "c_visit", "c_scale"}}: every search uses the Gumbel root (TreeSearch, gumbel).  The
    move is the root's argmax(g + logit + sigma(q)) -- the opening resampling of turns <= 6 does not apply, the Gumbel draw is
    the exploration -- and the recorded policy is the improved policy, through the same record route.  In lock step, with
    playout_cap (a quiet fast ply has g = 0 and is deterministic) and with rolling; one slot, no keep_tree.
    {"gumbel": True, "gumbel_interior": True} adds the Gumbel rule below the root (TreeSearch, gumbel_interior).
    {"solver": True}: proven wins and losses below the root (TreeSearch, solver): a game whose tree holds the finishing move
    plays it; the recorded policy stays the visit distribution.  In lock step, with playout_cap, rolling and keep_tree; not
    with gumbel."""

    def __init__(self, games, sims, evaluator, device=None, slots=1, seed=0, plane_dtype=None,
                 keep_records=True, game_ids=None, max_finished_kept=1024, report_every=0, log=print, packed_records=False,
                 search_options=None, playout_cap=None, rolling=None):
        import itertools
        from .batch import BoardBatch
        self.playout_cap = None
        if playout_cap is not None:
            cap = dict(playout_cap)
            unknown = set(cap) - {"full", "fast", "p_full", "quiet_fast"}
            if unknown or not {"full", "fast", "p_full"} <= set(cap):
                raise ValueError("playout_cap takes full, fast, p_full and optionally quiet_fast")
            cap["full"], cap["fast"], cap["quiet_fast"] = int(cap["full"]), int(cap["fast"]), bool(cap.get("quiet_fast", True))
            if cap["full"] < 1 or cap["fast"] < 1 or sims != max(cap["full"], cap["fast"]):
                raise ValueError("playout_cap: full and fast must be at least 1 and sims must equal max(full, fast)")
            cap["threshold"] = full_threshold(float(cap["p_full"]))
            if keep_records and not packed_records:
                raise ValueError("playout_cap with keep_records needs packed_records=True: the per-row tuples cannot carry "
                                 "the full / fast flag")
            self.playout_cap = cap
        self.games, self.sims, self.seed = games, sims, int(seed)
        self.env = BoardBatch(games, device)
        self.device = self.env.device
        self.rolling = rolling_options(rolling, search_options, sims, slots, self.playout_cap)
        self.search = TreeSearch(games, sims, evaluator, self.device.index, slots, seed, plane_dtype,
                                 **dict(search_options or {}, **({"rolling": True} if self.rolling else {})))
        # (search_options: e.g. skip_unread_rows / share_equal_leaves = False)
        # keep_tree: the action every slot stepped at the last ply (-3 = none: a new game, or the slot did not move)
        self._played = (torch.full((games,), -3, dtype=torch.int32, device=self.device) if self.search.keep_tree else None)
        self.keep_records = keep_records
        self.finished = 0
        self.white_wins = self.black_wins = self.draws = 0
        self.plies = 0
        self.finished_lengths = []   # mean final turn number of the games retired at one ply (bench statistics)
        self.finished_turns = []     # final turn number of every finished game
        self.records = []            # last 8 plies on the device: (features int64[games,144], policy, mover, game_id)
        self._ids = iter(game_ids) if game_ids is not None else itertools.count(0)
        first = [next(self._ids, -1) for _ in range(games)]
        self.game_id = torch.tensor(first, dtype=torch.int64, device=self.device)
        self.active = (self.game_id >= 0).to(torch.int8)
        self.search.set_game_ids(torch.clamp(self.game_id, min=0))
        # host copies of every ply still needed by a running game (features, history, policy, records, moved?)
        self._plylog = PlyLog(games, max_finished_kept)
        self._pinned_pool = []       # page-locked staging sets waiting to be reused (play_ply)
        self.finished_games = []     # finished games as tuples (packed_records=False)
        self.packed_records = bool(packed_records)
        self.finished_packed = []    # packed batches of finished games (packed_records=True)
        self.report_every, self._log_fn, self._reported = report_every, log, 0
        # per-ply record copies leave on a side stream into pinned host buffers while the next search runs
        self._copy_stream = torch.cuda.Stream(self.device) if keep_records else None
        self._copy_done = None       # event of the newest record copy (the log's entries are valid once it has passed)
        if self.playout_cap is not None:
            self.budget = torch.zeros((games,), dtype=torch.int32, device=self.device)
            self.full = torch.zeros((games,), dtype=torch.int8, device=self.device)
            self.quiet = torch.zeros((games,), dtype=torch.int8, device=self.device) if self.playout_cap["quiet_fast"] else None
        if self.rolling:
            dev = self.device
            if self.playout_cap is not None:
                # hive_search_draw_budgets draws every game (and zeroes the idle ones): into scratch, merged under the mask
                self._draw = (torch.zeros_like(self.budget), torch.zeros_like(self.quiet) if self.quiet is not None else None,
                              torch.zeros_like(self.full))
            else:
                self.budget, self.quiet = torch.full((games,), sims, dtype=torch.int32, device=dev), None
            self.search.set_budgets(self.budget, self.quiet)
            assert self.search._budgets.data_ptr() == self.budget.data_ptr()        # the handle reads THESE arrays at every select
            self._root_boards = torch.zeros((games, 64), dtype=torch.uint8, device=dev)
            self._root_hist = torch.zeros((games, 384), dtype=torch.uint8, device=dev)
            self._restart = torch.ones((games,), dtype=torch.bool, device=dev)      # slots whose next search starts at the next turn-over

    def stagger(self, seed=0):
        """Spread the games over plies 0..53 with uniformly random legal moves so that a timed window
        sees the steady state.  Those opening plies are not searched and not logged, so the
        games they belong to produce no training rows (their [game_len, counter] would be wrong)."""
        from .playout import pick_uniform
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        target = torch.randint(0, MAX_GAME_LENGTH - 1, (self.games,), device=self.device, generator=gen)
        for ply in range(MAX_GAME_LENGTH - 1):
            over, _ = self.env.terminal()
            _, count, lst = self.env.legal(want_list=True)
            a = pick_uniform(count, lst, gen)
            go = (target > ply) & (over == 0) & (self.active != 0)
            self.env.step(torch.where(go, a, torch.full_like(a, -2)), sync=False)
        self._plylog.unlogged = [bool(t > 0) for t in target.cpu().tolist()]

    def running(self):
        """Number of slots that still hold a game."""
        return int(self.active.sum().item())

    def _retire_finished(self):
        boards, _ = self.env.export_state()
        over, winner = self.env.terminal()
        turn = boards[:, 33].to(torch.int32)
        done = ((over != 0) | (turn >= MAX_GAME_LENGTH)) & (self.active != 0)
        nd = int(done.sum().item())
        if nd:
            w = winner[done]
            self.white_wins += int((w == 1).sum().item())
            self.black_wins += int((w == 2).sum().item())
            self.draws += int((w == 0).sum().item())
            self.finished += nd
            self.finished_lengths.append(turn[done].float().mean().item())
            self.finished_turns += turn[done].cpu().tolist()
            idx = torch.nonzero(done).view(-1).to(torch.int32)
            slots = idx.cpu().tolist()
            if self.keep_records:
                self._close_games(slots, winner.cpu().tolist(), self.game_id.cpu().tolist())
            fresh = [next(self._ids, -1) for _ in slots]
            for sl, f in zip(slots, fresh):
                if f < 0:
                    self._plylog.idle(sl)
            self.game_id[idx.long()] = torch.tensor(fresh, dtype=torch.int64, device=self.device)
            self.active = (self.game_id >= 0).to(torch.int8)
            self.search.set_game_ids(torch.clamp(self.game_id, min=0))
            self.env.reset(idx)
            if self._played is not None:
                self._played[idx.long()] = -3               # the slot's next search belongs to another game
            self._report()
        return nd

    retire_finished = _retire_finished

    def _report(self):
        """woker/self_play.py:69-75: every `report_every` games -- games so far, mean game length, white's win rate."""
        if self.report_every and self.finished - self._reported >= self.report_every:
            self._reported = self.finished - self.finished % self.report_every
            self._log_fn(f" Total_game {self.finished} ---  Mean_game_len {self.mean_game_length():.2f} ---  "
                         f"White_Win % {self.white_wins / max(self.finished, 1):.2f} ---  "
                         f"(white {self.white_wins} black {self.black_wins} draw_or_cap {self.draws})")

    def mean_game_length(self):
        """Mean number of plies of the finished games (final turn number - 1)."""
        return (sum(self.finished_turns) / len(self.finished_turns) - 1.0) if self.finished_turns else 0.0

    def _log_ready(self):
        """Wait for the newest per-ply record copy (issued a whole search ago: it has long finished)."""
        if self._copy_done is not None:
            self._copy_done.synchronize()

    def _close_games(self, slots, winner, ids):
        """The games that ended leave the log as one packed batch, kept as it is or expanded game by game."""
        self._log_ready()
        waiting = len(self.finished_games) + sum(packed_games(b) for b in self.finished_packed)
        packed = self._plylog.close_games(slots, winner, ids, self.plies, waiting)
        if packed is not None and self.packed_records:
            self.finished_packed.append(packed)
        elif packed is not None:
            self.finished_games += [unpack_game(packed, g) for g in range(packed_games(packed))]

    dropped_games = property(lambda self: self._plylog.dropped_games)
    unrecorded_games = property(lambda self: self._plylog.unrecorded_games)

    def drain_finished(self):
        """Take (and forget) every finished game collected so far: list of (value_white, plies, game_id);
        `game_rows(entry)` turns one into the reference's rows."""
        out, self.finished_games = self.finished_games, []
        return out

    def drain_finished_packed(self):
        """packed_records=True: take (and forget) the finished games collected so far as ONE packed batch
        (records.pack_games' arrays; records.unpack_game / PackedGames expand them), or None if there are none."""
        batches, self.finished_packed = self.finished_packed, []
        return concat_packed(batches) if batches else None

    ply_record = staticmethod(PlyLog.ply_record)    # (entry of the log, slot) -> one ply tuple

    def last_ply_record(self, g):
        self._log_ready()
        log = self._plylog.entries
        return self.ply_record(log[-1], g) if log and log[-1]["moved"][g] else None

    game_rows = staticmethod(rows_from_game)        # one finished game -> the reference's JSON rows

    def finished_game_rows(self, k):
        """The k-th waiting finished game as the reference's rows."""
        return self.game_rows(self.finished_games[k])

    def _draw_budgets(self, boards, budget, quiet, full):
        """Every game's ply at `boards` drawn full or fast from (seed, game id, turn) into budget / quiet / full
        (hive_search_draw_budgets; idle games get zeros)."""
        cap = self.playout_cap
        check(self.search.L.hive_search_draw_budgets(ctypes.c_uint64(self.seed & (2 ** 64 - 1)), _p(self.game_id), _p(boards),
                                                     _p(self.active), self.games, cap["full"], cap["fast"], cap["threshold"],
                                                     _p(budget), _p(quiet), _p(full), stream_ptr(self.device)))

    def _log_ply(self, feat, policy, boards, hist, action):
        """The record route, the only place that issues a record copy: the searched positions (packed features, boards,
        history), the policies and who moved (action != -2) of this ply join the `records` ring and leave for the log."""
        mover = (1 - (boards[:, 33] & 1)).to(torch.int8)
        # (the rolling search's root_feat is rewritten in place at the next turn-over; root_planes is a fresh clone per search)
        self.records.append((feat.clone() if self.rolling else feat, policy.clone(), mover, self.game_id.clone()))
        if len(self.records) > 8:
            self.records.pop(0)
        # host copies of this ply for the per-game records (8 MB per ply at 1024 games; whole arrays, the per-game
        # rows are cut out only when a game ends: PlyLog).  They leave asynchronously: a side stream copies into pinned
        # buffers while the main stream goes on with the env step and the next search (self_play.py:159-160 appends a
        # row per ply in the game loop itself; here that costs the engine nothing but the PCIe transfer)
        src = {"feat": feat, "policy": policy, "boards": boards, "hist": hist, "moved": action != -2}
        if self.playout_cap is not None:
            src["full"] = self.full             # (redrawn by the next ply, which waits for this copy like the policy buffer)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        prev_copy = self._copy_done
        # page-locked staging buffers are recycled: a ply's arrays move to pageable memory one ply later (settle), so
        # two or three sets exist per engine instead of one per ply of the longest running game (8-32 MB each)
        host = self._pinned_pool.pop() if self._pinned_pool else \
            {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in src.items()}
        with torch.cuda.stream(self._copy_stream):
            self._copy_stream.wait_event(ready)
            for k, v in src.items():
                host[k].copy_(v, non_blocking=True)
                v.record_stream(self._copy_stream)
            self._copy_done = torch.cuda.Event()
            self._copy_done.record(self._copy_stream)
        # (the arrays are views of the pinned tensors: `host` travels along as the entry's keepalive)
        log = self._plylog
        log.append(self.plies, keepalive=host, **{k: v.numpy() for k, v in host.items()})
        if len(log.entries) >= 2 and prev_copy is not None:
            # the previous ply's copy was issued a whole search ago: its sparse policies are built now, while the GPU
            # runs this ply's search (the host has nothing else to do), not when a thousand games end at once
            prev_copy.synchronize()
            freed = log.settle(log.entries[-2])
            if freed is not None:
                self._pinned_pool.append(freed)

    def play_ply(self, forced=None):
        """One move for every game.  Returns the number of games that finished before this move.
        forced: optional int32[games]; entries >= -1 replace the searched move of that slot (replaying a recorded game
        through the record path; -2 = keep the search's choice).
        rolling: one turn-over -- the games whose search is complete move, the others go on searching (class docstring)."""
        if self.rolling:
            return self._play_turnover(forced)
        nd = self._retire_finished()
        boards, hist = self.env.export_state()
        if self._copy_done is not None:
            # the search's policy buffer is rewritten at the end of this search: it waits for the previous ply's record copy
            torch.cuda.current_stream(self.device).wait_event(self._copy_done)
        extra = {}
        if self._played is not None:
            extra["played"] = self._played
        if self.playout_cap is not None:
            self._draw_budgets(boards, self.budget, self.quiet, self.full)
            extra["budgets"], extra["quiet"] = self.budget, self.quiet
        action, policy, sum_n = self.search.search(boards, hist, active=self.active, selfplay=True,
                                                   keep_root_planes=self.keep_records, **extra)
        if self.keep_records:
            self._log_ply(self.search.root_planes.view(self.games, 144), policy, boards, hist, action)
        action = _override(action, forced)
        # the env re-derives the legal masks and refuses anything not in them: the search's edges come
        # from the same kernels, so illegal_count() must stay 0 (asserted by the tests)
        self.env.step(action, sync=False)
        if self._played is not None:
            self._played = torch.where(action == -2, torch.full_like(action, -3), action)
        self.plies += 1
        return nd

    def _play_turnover(self, forced=None):
        """play_ply() of the rolling engine."""
        G, search = self.games, self.search
        nd = self._retire_finished()
        boards, hist = self.env.export_state()
        if self._copy_done is not None:
            # the policy, root and flag buffers are rewritten below: they wait for the previous turn-over's record copy
            torch.cuda.current_stream(self.device).wait_event(self._copy_done)
        # the games that moved at the last turn-over, and the slots that took a new game since (they moved too: a game ends
        # by a move), draw their budgets and start their next search; every other game keeps its own
        w = self._restart
        if self.playout_cap is not None:
            budget, quiet, full = self._draw
            self._draw_budgets(boards, budget, quiet, full)
            torch.where(w, budget, self.budget, out=self.budget)
            torch.where(w, full, self.full, out=self.full)
            if quiet is not None:
                torch.where(w, quiet, self.quiet, out=self.quiet)
        torch.where(w.view(G, 1), boards, self._root_boards, out=self._root_boards)
        torch.where(w.view(G, 1), hist, self._root_hist, out=self._root_hist)
        search.restart(w, self._root_boards, self._root_hist, self.active)
        done = search.run_rounds(self.rolling["quantum"], keep_root_planes=self.keep_records)
        action, policy, sum_n = search.policy_where(done, selfplay=True)
        if self.keep_records:
            # the entry holds the roots the finished searches started from
            self._log_ply(search.root_feat, policy, self._root_boards, self._root_hist, action)
        action = _override(action, forced)
        self.env.step(action, sync=False)
        self._restart = action != -2
        self.plies += 1
        return nd

    def leaf_histogram(self):
        """{kind: count} over every simulation since create (TreeSearch.leaf_histogram summed over the games)."""
        h = self.search.leaf_histogram().sum(0).cpu().tolist()
        return {k: int(v) for k, v in zip(LEAF_KINDS, h) if k != "unused"}

    def close(self):
        self.search.close()
        self.env.close()
