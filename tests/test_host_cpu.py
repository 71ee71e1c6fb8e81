"""CPU-only checks: the C-ABI library loads and exports every declared symbol, host packing / record helpers, the
test-side checkers (UCT restatement, caller drivers) and the sequential HivePlayer mirror against the reference's
golden outputs (driven by the oracle env = BASELINE config C1), and the world-size-2 sharding path over gloo."""
import gzip
import json
import os
import re
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_abi_library_exports_every_declared_symbol():
    import hive_alphazero_amd as h
    from hive_alphazero_amd import _lib
    h.build()
    L = h.load()
    declared = []
    for hdr in ("hive_abi.h", "hive_search.h", "hive_nn.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        declared += re.findall(r"\b(hive_[a-z_0-9]+)\s*\(", text)
    declared = sorted(set(declared))
    assert len(declared) >= 28
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/ but not exported"
    assert sorted(set(_lib.ABI_SYMBOLS)) == declared
    assert L.hive_version().startswith(b"hive-hip")


def test_abi_headers_are_plain_c(tmp_path):
    """include/*.h compile as C with gcc (struct sizes pinned by _Static_assert) and the HIVE_MASK_* macros address
    the legal-set words exactly like the host-side packing helpers."""
    exe = tmp_path / "abi_header_check"
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "abi_header_check.c"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "0"
    from hive_alphazero_amd import packing
    ids = [0, 11, 131, 132, 858, 1583]
    m = packing.actions_to_mask(ids)
    for a in range(1584):
        cell, slot = divmod(a, 11)
        row, col = divmod(cell, 12)
        assert bool((int(m[slot * 6 + (row >> 1)]) >> (((row & 1) << 4) | col)) & 1) == (a in ids)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ctypes
    import hive_alphazero_amd as h
    L = h.load()
    hd = ctypes.c_void_p()
    assert L.hive_batch_create(4, 0, ctypes.byref(hd)) == -2
    assert b"no HIP device" in L.hive_last_error()
    from hive_alphazero_amd.batch import BoardBatch
    with pytest.raises(h.HiveError):
        BoardBatch(4)


def test_packing_roundtrip(golden_games):
    from hive_alphazero_amd import packing
    recs = [r for g in golden_games[:5] for r in g["plies"]]
    turn = np.array([r["t"] for r in recs])
    pos = np.array([r["pos"] for r in recs], dtype=np.uint8)
    lvl = np.array([r["lvl"] for r in recs], dtype=np.uint8)
    rec = packing.pack_boards(turn, pos, lvl, np.zeros(len(recs), dtype=np.uint8))
    st = packing.unpack_boards(rec)
    assert st["turn"].tolist() == turn.tolist() and np.array_equal(st["pos"], pos) and np.array_equal(st["lvl"], lvl)
    assert packing.words_to_cells(packing.mask_words([0, 13, 143, 77])) == [0, 13, 77, 143]
    ids = [0, 31, 32, 858, 1583]
    m = packing.actions_to_mask(ids)
    assert m.shape == (66,) and packing.mask_to_actions(m) == ids
    assert int(m[0]) == 1 and int(m[10 * 6 + 5]) == 1 << (16 + 11)      # (slot 0, cell 0) and (slot 10, cell 143)


def test_records_wire_format(tmp_path, golden_games):
    from hive_alphazero_amd import records
    rec = golden_games[0]["plies"][12]
    words = np.zeros(144, dtype=np.uint64)
    for idx in rec["planes"]:
        cell, p = divmod(idx, 56)
        if not 36 <= p < 44:
            words[cell] |= np.uint64(1) << np.uint64(p)
    hist = np.zeros((12, 12, 8))
    for idx in rec["planes"]:
        cell, p = divmod(idx, 56)
        if 36 <= p < 44:
            hist[cell // 12, cell % 12, p - 36] = 1
    planes = records.unpack_features(words, rec["t"], hist)
    want = np.zeros((12, 12, 56))
    want.reshape(-1)[rec["planes"]] = 1
    want[:, :, 31] = rec["t"]
    assert np.array_equal(planes, want)
    pol = np.zeros(1584)
    pol[rec["legal"][0]] = 1.0
    rows = records.game_entries([(planes, pol, "W"), (planes, pol, "B"), (planes, pol, "W")], value_white=1)
    assert [r[2] for r in rows] == [1, -1, 1] and [r[3] for r in rows] == [[2, 1], [1, 1], [2, 2]]
    assert [r[2] for r in records.game_entries([(planes, pol, "W"), (planes, pol, "B")], 0)] == [-1, -1]
    path = records.flush_buffer(rows, str(tmp_path))
    back = records.load_data(path)
    assert len(back) == 3 and back[0][0].shape == (12, 12, 56)
    assert back[0][2] == pytest.approx(1 * 0.99 ** (2 - 1)) and back[2][2] == 1     # optimize.py:55-58


@pytest.mark.parametrize("fixture", ["uct.json", "uct_deep.json"])
def test_uct_restatement_matches_reference(fixture):
    """tests/uct_ref.py (the checker the GPU tests hold the HIVE_SEARCH_UCT kernels against) reproduces the TRUE reference's
    UCTNode search (oracle/gen_golden.py uct [--deep]): visits, total values and the chosen move -- 40 reads from early
    positions, 120 reads from late ones (deeper trees, finished games inside the tree, a finished game as the root)."""
    from mcts_stub import stub_predict
    from oracle_env import OracleGamePlay
    from uct_ref import uct_reads
    with open(os.path.join(GOLD, fixture)) as f:
        gold = json.load(f)
    for case in gold["cases"]:
        g = OracleGamePlay()
        for a in case["prefix"]:
            g.move(a)
        N, W, _, best = uct_reads(g, case["reads"], stub_predict)
        assert [[int(i), float(N[i]), float(W[i])] for i in np.nonzero(N)[0]] == case["visits"]
        assert best == case["best"]


def test_selfplay_golden_through_the_sequential_search():
    """BASELINE config C1: one whole self-play game (sequential HivePlayer mirror, stub evaluator, CPU env) against the
    rows the TRUE reference's self_play_buffer wrote (tests/golden/selfplay.json.gz); the caller loop itself is the
    test-side driver tests/caller_harness.py."""
    import hive_alphazero_amd.solo_play as sp
    from caller_harness import selfplay_game
    from mcts_stub import StubPipe
    from oracle_env import OracleGamePlay
    with gzip.open(os.path.join(GOLD, "selfplay.json.gz"), "rt") as f:
        gold = json.load(f)
    sp.SEARCH_THREADS = 1
    np.random.seed(gold["seed"])
    pipes = [StubPipe()]
    players = [sp.HivePlayer(pipes=pipes), sp.HivePlayer(pipes=pipes)]
    data, value_white = selfplay_game(OracleGamePlay(), lambda side: players[side], sims=gold["sims"])
    assert [value_white] == gold["value_white"]
    assert len(data) == len(gold["rows"])
    for (state, policy, value, lens), row in zip(data, gold["rows"]):
        arr = np.asarray(state, dtype=np.float32)
        assert int(zlib.crc32(arr.tobytes())) == row["crc"]
        assert [[i, float(x)] for i, x in enumerate(policy) if x != 0] == row["pol"]
        assert value == row["v"] and lens == row["lens"]


_WORKER = r"""
import os, sys, json, gzip
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch.distributed as dist
from hive_alphazero_amd import dist as hd
from oracle import oracle_py as O
rank, local_rank, world = hd.init("gloo")
with gzip.open(os.path.join(sys.argv[1], "tests", "golden", "games_movegen.json.gz"), "rt") as f:
    recs = [r for g in json.load(f)["games"][:8] for r in g["plies"]]
lo, hi = hd.shard(len(recs), rank, world)
mine = recs[lo:hi]
total, _ = O.batch_legal([r["t"] for r in mine], [r["pos"] for r in mine], [r["lvl"] for r in mine],
                         [1 if r["t"] == 1 else 2 if r["t"] == 2 else 0 for r in mine], want_masks=False)
want = sum(len(r["legal"]) for r in mine)
assert total == want, (rank, total, want)
hd.barrier()
all_total = hd.sum_over_ranks(total)
all_units = hd.sum_over_ranks(hi - lo)
slowest = hd.max_over_ranks(1.0 + rank)
if rank == 0:
    print(json.dumps({"total": all_total, "units": all_units, "n": len(recs), "slowest": slowest,
                      "want": sum(len(r["legal"]) for r in recs)}))
dist.destroy_process_group()
"""


def test_sharding_world_size_2_gloo(tmp_path):
    """The N>1 path of bench.py on CPU: units sharded by rank, no data-path collective, barrier +
    scalar reductions only; the shards' results add up to the whole."""
    from hive_alphazero_amd import dist as hd
    assert [hd.shard(10, r, 3) for r in range(3)] == [(0, 4), (4, 7), (7, 10)]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29577", str(script), ROOT],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert res["total"] == res["want"] and res["units"] == res["n"] and res["slowest"] == 2.0


def test_recorded_game_golden_on_the_cpu_env():
    """The reference's SL ingest rows (tests/golden/sl.json.gz: a finished game with bot-weighted moves, a game with an
    out-of-turn step that triggers skip_turn, an unfinished prefix) replayed step by step over the CPU oracle env."""
    from caller_harness import replay_recorded_game
    from oracle_env import OracleGamePlay
    with gzip.open(os.path.join(GOLD, "sl.json.gz"), "rt") as f:
        gold = json.load(f)
    for case in gold["cases"]:
        data = replay_recorded_game(OracleGamePlay(), case["steps"])
        assert len(data) == len(case["rows"]) > 0
        for (state, policy, value, lens), row in zip(data, case["rows"]):
            assert int(zlib.crc32(np.asarray(state, dtype=np.float32).tobytes())) == row["crc"]
            assert [[i, float(x)] for i, x in enumerate(policy) if x != 0] == row["pol"]
            assert value == row["v"] and lens == row["lens"]


def test_sl_schedule_host_logic():
    """hive_alphazero_amd.sl: step decoding and the host-side replay plan (no GPU)."""
    from hive_alphazero_amd import sl
    assert sl.decode_piece("Q") == "<class 'pieces.Queen'>0" and sl.decode_piece("G3") == "<class 'pieces.Grasshopper'>2"
    assert sl.step_action(["Q", "N", "13", "W", 0]) == 858           # Start_Tile ('N','13') = cell 78, slot 0
    plan = sl._schedule([["Q", "N", "13", "W", 0], ["A1", "M", "13", "B", 1], ["A2", "M", "12", "B", 0]])
    assert [p[0] for p in plan] == [False, False, True]              # black moving twice in a row needs a skip
    assert [p[4] for p in plan] == [1, 1, 2] and plan[1][3] is True


@pytest.fixture
def no_device_mask(monkeypatch):
    """For the SelfPlayWorker tests whose stand-in children touch no GPU: they name logical GPUs 0..7, and a device mask
    inherited from a scheduler (one entry on a one-GPU host) would only decide whether those exist.  The translation
    through such a mask is test_selfplay_worker_device_masks_and_lost_games' subject, which sets its own."""
    monkeypatch.delenv("HIP_VISIBLE_DEVICES", raising=False)
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)


def test_selfplay_worker_shards_games_by_global_id(tmp_path, no_device_mask):
    """SURVEY 8e / woker/self_play.py:37-75,100-112: SelfPlayWorker spawns one child per GPU (HIP_VISIBLE_DEVICES set for the
    child before it starts), hands rank r the contiguous shard of the global game ids, gathers the finished games, prints
    the progress line every 10 games and flushes rows every N games.  With a GPU-free stand-in worker at world size 2:
    every game id is played exactly once on the right device, and the merged result equals the world-size-1 result."""
    import itertools
    import fake_selfplay_worker as fw
    from hive_alphazero_amd import dist as hd
    from hive_alphazero_amd.self_play import SelfPlayWorker
    # rank -> game ids: contiguous shards of a fixed total; strided when open-ended; unique across ranks either way
    assert [list(hd.game_id_stream(r, 3, 10)) for r in range(3)] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    opened = [list(itertools.islice(hd.game_id_stream(r, 4), 3)) for r in range(4)]
    assert opened == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
    runs = {}
    for gpus in ([0], [0, 1]):
        lines = []
        w = SelfPlayWorker(total_games=23, games_per_gpu=4, sims=2, gpus=gpus, seed=7, datapath=str(tmp_path / f"w{len(gpus)}"),
                           games_per_file=10, report_every=10, worker=fw.worker, log=lines.append)
        res = w.start(timeout_s=120)
        assert list(res) == list(range(23))
        lo1 = hd.shard(23, 1, len(gpus))[0] if len(gpus) > 1 else 23
        for g, (vw, rows) in res.items():
            assert rows[0][0][2] == ("0" if g < lo1 else "1")          # the child saw exactly its own GPU
            rows[0][0].pop()
            assert (vw, rows) == fw.fabricate(7, g)
        assert len(lines) == 2 and lines[0].startswith(" Total_game 10 ---") and "White_Win %" in lines[1]
        assert len(w.files) == 3 and w.leaf_kinds == {"root_evaluated": 23}   # 10 + 10 + the final partial flush
        data = [r for f in w.files for r in json.load(open(f))]
        assert len(data) == sum(len(rows) for _, rows in res.values())
        runs[len(gpus)] = res
    assert runs[1] == runs[2]
    assert "HIP_VISIBLE_DEVICES" not in os.environ or os.environ["HIP_VISIBLE_DEVICES"] != "1"


def test_selfplay_worker_device_masks_and_lost_games(tmp_path, monkeypatch):
    """The child's device mask is the parent's logical index translated through whatever mask the parent inherited
    (a scheduler's HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES = "4,5,6,7"), applied by the child itself, the parent's
    environment untouched; a rank that drops a game -- loudly or silently -- fails the run instead of returning fewer
    games than promised (self_play.py docstring: 'games 0 .. total_games-1')."""
    import fake_selfplay_worker as fw
    from hive_alphazero_amd.self_play import SelfPlayWorker, child_device_env
    assert child_device_env(1, {}) == {"HIP_VISIBLE_DEVICES": "1", "CUDA_VISIBLE_DEVICES": None}
    assert child_device_env(2, {"HIP_VISIBLE_DEVICES": "4,5,6,7"})["HIP_VISIBLE_DEVICES"] == "6"
    assert child_device_env(0, {"CUDA_VISIBLE_DEVICES": "3, 1"})["HIP_VISIBLE_DEVICES"] == "3"
    assert child_device_env(1, {"HIP_VISIBLE_DEVICES": "7,2", "CUDA_VISIBLE_DEVICES": "0,1"})["HIP_VISIBLE_DEVICES"] == "2"
    with pytest.raises(RuntimeError):
        child_device_env(2, {"HIP_VISIBLE_DEVICES": "4,5"})
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "5,3")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "0,1")
    w = SelfPlayWorker(total_games=9, games_per_gpu=4, sims=2, gpus=[0, 1], seed=7, datapath=None, games_per_file=0,
                       report_every=0, worker=fw.worker, log=lambda *_: None)
    res = w.start(timeout_s=120)
    lo1 = 5                                                   # shard(9, 1, 2)
    assert [rows[0][0][2] for _, (vw, rows) in sorted(res.items())] == ["5" if g < lo1 else "3" for g in range(9)]
    assert os.environ["HIP_VISIBLE_DEVICES"] == "5,3" and os.environ["CUDA_VISIBLE_DEVICES"] == "0,1"
    for seed in (666, 667):
        w = SelfPlayWorker(total_games=9, games_per_gpu=4, sims=2, gpus=[0, 1], seed=seed, datapath=None, games_per_file=0,
                           report_every=0, worker=fw.worker, log=lambda *_: None)
        with pytest.raises(RuntimeError, match="games lost"):
            w.start(timeout_s=120)


def test_compact_game_files_expand_to_the_reference_rows(tmp_path):
    """records.save_games / load_games keep finished games as they leave the GPU (packed 56-bit features, history bitboards,
    sparse policy); rows_from_game and dataset_from_games must yield exactly what the JSON route (game_entries ->
    flush_buffer -> load_data = woker/optimize.py:42-65) yields: same planes, same policies, same discounted values."""
    from hive_alphazero_amd import records
    rng = np.random.default_rng(0)
    games = []
    for gid, (vw, n) in enumerate(((1, 7), (0, 4), (-1, 9))):
        plies = []
        for k in range(n):
            words = rng.integers(0, 1 << 56, size=144, dtype=np.uint64) & ~np.uint64(1 << 31) & ~np.uint64(0xFF << 36)
            hist = rng.integers(0, 1 << 12, size=(4, 2, 6), dtype=np.uint32)
            policy = np.zeros(1584, dtype=np.float32)
            idx = rng.choice(1584, size=int(rng.integers(1, 40)), replace=False)
            policy[idx] = rng.random(len(idx)).astype(np.float32)
            policy /= policy.sum()
            plies.append((words, hist, min(k // 2, 4), k + 1, policy, k % 2))
        games.append((vw, plies, 100 + gid))
    path = records.save_games(str(tmp_path / "play.npz"), games)
    assert os.path.getsize(path) < 3000 * sum(len(g[1]) for g in games)
    back = records.load_games(path)
    assert [(g[0], len(g[1]), g[2]) for g in back] == [(g[0], len(g[1]), g[2]) for g in games]
    rows = [r for g in games for r in records.rows_from_game(g)]
    rows_back = [r for g in back for r in records.rows_from_game(g)]
    assert json.dumps(rows) == json.dumps(rows_back)
    json_path = records.flush_buffer(rows, str(tmp_path))
    via_json = records.load_data(json_path)                 # [state, policy, discounted value] per row
    states, policies, values = records.dataset_from_games(back)
    assert len(via_json) == len(states) == 20
    for (s, p, v), s2, p2, v2 in zip(via_json, states, policies, values):
        assert np.array_equal(s.astype(np.float32), s2) and np.array_equal(p, p2) and abs(v - v2) < 1e-6


def test_bench_gpus_flag_starts_the_ranks_itself(monkeypatch):
    """bench.py --gpus N (driver contract): without RANK in the environment the process starts N ranks under
    torch.distributed.run as a CHILD (before anything touches the GPU), forwards its argv, relays the child's exit code;
    with WORLD_SIZE set and different from --gpus it refuses to run.  (woker/self_play.py:54-56 is the reference's pool.)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import importlib
    bench = importlib.import_module("bench")
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 7)
    rc = bench.relaunch_under_torchrun(["--gpus", "4", "--steps", "5", "--dist-backend", "gloo"], 4)
    (cmd, env), = calls
    assert rc == 7 and cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "5", "--dist-backend", "gloo"]
    assert os.path.basename(cmd[cmd.index("--master-port") + 2]) == "bench.py" and env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.undo()
    # a rank count that contradicts the launcher's is refused before any import of torch
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    # no launcher on the command line: two ranks come up under torchrun (here they stop at "needs a GPU": this container has none)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--steps", "2",
                        "--warmup", "1"], env=env, capture_output=True, text=True, timeout=600)
    import torch
    if not torch.cuda.is_available():
        # (the launcher tears the other rank down as soon as the first one exits: one or both messages appear)
        assert r.returncode != 0 and r.stderr.count("bench.py needs a GPU") >= 1 and "torch.distributed" in r.stderr, r.stderr[-2000:]
    else:
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert r.returncode == 0 and line["n_gpus"] == 2


def test_packed_game_batches_round_trip_slice_and_concat(tmp_path):
    """records.pack_games / unpack_game / slice_packed / concat_packed / PackedGames: the array form of finished games that
    SelfPlayWorker's children send and play_<ts>.npz holds.  Packing, cutting into per-game slices, concatenating in another
    order and expanding again must give back every game exactly; an empty batch and a game with an all-zero policy row
    (a forced pass) included."""
    from hive_alphazero_amd import records
    rng = np.random.default_rng(4)

    def game(gid, plies):
        rows = []
        for t in range(plies):
            pol = np.zeros(1584, np.float32)
            k = int(rng.integers(0, 30))
            pol[rng.choice(1584, k, replace=False)] = rng.random(k).astype(np.float32) + 0.01
            rows.append((rng.integers(0, 2 ** 56, 144, dtype=np.uint64), rng.integers(0, 2 ** 28, (4, 2, 6), dtype=np.uint32) & np.uint32(0x0FFF0FFF),
                         int(rng.integers(0, 5)), t + 1, pol, t & 1))
        return (int(rng.integers(-1, 2)), rows, gid)

    def same(a, b):
        assert a[0] == b[0] and a[2] == b[2] and len(a[1]) == len(b[1])
        for x, y in zip(a[1], b[1]):
            assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(x, y))

    games = [game(7, 5), game(3, 1), game(11, 9), game(0, 4)]
    packed = records.pack_games(games)
    assert records.packed_games(packed) == 4 and packed["game_ptr"].tolist() == [0, 5, 6, 15, 19]
    for g, entry in enumerate(games):
        same(records.unpack_game(packed, g), entry)
    parts = [records.slice_packed(packed, g, g + 1) for g in (2, 0, 3, 1)]
    again = records.concat_packed(parts)
    assert again["game_id"].tolist() == [11, 7, 0, 3] and again["pol_ptr"][-1] == len(again["pol_idx"]) == len(packed["pol_idx"])
    for g, src in enumerate((2, 0, 3, 1)):
        same(records.unpack_game(again, g), games[src])
    same(records.unpack_game(records.slice_packed(packed, 1, 3), 1), games[2])
    empty = records.pack_games([])
    assert records.packed_games(empty) == 0 and records.packed_games(records.concat_packed([])) == 0
    both = records.concat_packed([empty, packed, empty])
    assert both["game_ptr"].tolist() == packed["game_ptr"].tolist()
    path = records.save_packed(str(tmp_path / "g.npz"), again)
    for a, b in zip(records.load_games(path), (games[2], games[0], games[3], games[1])):
        same(a, b)
    view = records.PackedGames()
    view.add(records.slice_packed(packed, 0, 2))
    view.add(records.slice_packed(packed, 2, 4))
    view.sort()
    assert list(view) == [0, 3, 7, 11] and len(view) == 4 and 7 in view and 5 not in view
    assert view.rows_of(11) == 9
    same(view[11], games[2])
    assert [k for k, _ in view.items()] == [0, 3, 7, 11]
    # the trainer's values (optimize.py:42-65 discount) straight from the packed arrays == the row-wise rule
    assert np.array_equal(records.packed_values(packed), records.dataset_from_games(games)[2])
    # ... == the reference's own rule: its rows (game_entries) written to a play_<ts>.json and loaded back (load_data)
    rows = [r for vw, plies, _ in games
            for r in records.game_entries([(np.zeros((1, 1, 1)), p[4], "W" if p[5] == 0 else "B") for p in plies], vw)]
    loaded = records.load_data(records.flush_buffer(rows, str(tmp_path / "json")))
    assert np.array_equal(records.packed_values(packed), np.asarray([r[2] for r in loaded], dtype=np.float32))


def test_selfplay_worker_takes_packed_batches_from_two_ranks(tmp_path, no_device_mask):
    """The compact route at world size 2 without a GPU: children send packed batches of several games per message
    (records.pack_games' arrays); the parent cuts files at exactly games_per_file games on writer threads, `results` is a
    lazy game-id mapping, and files + mapping hold every game exactly as fabricated."""
    import fake_selfplay_worker as fk
    from hive_alphazero_amd import records
    from hive_alphazero_amd.self_play import SelfPlayWorker
    w = SelfPlayWorker(total_games=23, games_per_gpu=4, sims=1, gpus=[0, 1], seed=3, datapath=str(tmp_path), games_per_file=5,
                       report_every=0, worker=fk.packed_worker, log=lambda *_: None, row_format="compact")
    res = w.start(timeout_s=120)
    assert isinstance(res, records.PackedGames) and list(res) == list(range(23))
    assert len(w.files) == 5 and all(os.path.exists(f) for f in w.files)          # 4 x 5 games + the last 3
    loaded = [g for f in w.files for g in records.load_games(f)]
    assert [len(records.load_games(f)) for f in w.files] == [5, 5, 5, 5, 3]
    assert sorted(g[2] for g in loaded) == list(range(23))
    assert sum(w.game_lens) == sum(len(g[1]) for g in loaded) and len(w.win_lose) == 23
    for entry in loaded:
        want = fk.fabricate_compact(3, entry[2])
        for got in (entry, res[entry[2]]):
            assert got[0] == want[0] and len(got[1]) == len(want[1])
            for x, y in zip(got[1], want[1]):
                assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(x, y))


def test_selfplay_worker_parent_keeps_up_with_eight_ranks_of_real_size_waves(tmp_path, no_device_mask):
    """The ONE serial point of the 8-GPU producer (woker/self_play.py:37-75,100-112: one parent gathers every game and writes
    the files): eight ranks hand over real-size lock-step waves -- 1024 games = 55 k rows = ~90 MB per message, as
    mcts.SelfPlay.drain_finished_packed sends them -- at 8 x 4,700 games/min (one wave per rank every 13 s, all ranks at the
    same moment: the worst burst).  The parent must keep the backlog bounded, land every game id exactly once, cut every
    file at exactly games_per_file games, and be done shortly after the last wave left.  HIVE_SOAK_PARENT_WAVES=5 soaks it
    for a minute; the default (2 waves) keeps the CPU suite short."""
    import fake_selfplay_worker as fk
    from hive_alphazero_amd import records
    from hive_alphazero_amd.self_play import SelfPlayWorker
    ranks, per_wave = 8, 1024
    waves = int(os.environ.get("HIVE_SOAK_PARENT_WAVES", "2"))
    period_s = per_wave / 4700.0 * 60.0                        # 13.07 s: one GPU's wave period at 4,700 games/min
    total = ranks * per_wave * waves
    spool = os.environ.get("HIVE_SPOOL_DIR", "/dev/shm")       # shared with other runs on the host: only this run's files count
    parked_before = {f for f in os.listdir(spool) if f.startswith("hive_wave_")}
    w = SelfPlayWorker(total_games=total, games_per_gpu=per_wave, sims=1, gpus=list(range(ranks)), seed=5,
                       slots=int(period_s * 1000), datapath=str(tmp_path), games_per_file=256, report_every=0,
                       worker=fk.soak_worker, log=lambda *_: None, row_format="compact", keep_results=False)
    t0 = time.time()
    res = w.start(timeout_s=600)
    t1 = time.time()
    ready = max(w.ready_at.values())
    last_wave_sent = ready + (waves - 1) * period_s
    assert isinstance(res, records.PackedGames) and len(res) == total and list(res)[:3] == [0, 1, 2] and list(res)[-1] == total - 1
    assert res.rows_of(total - 1) == 54                         # keep_results=False: ids and lengths stay, the rows are in the files
    with pytest.raises(KeyError):
        res[0]
    assert not [f for f in os.listdir(spool) if f.startswith("hive_wave_") and f not in parked_before]   # nothing left parked
    # the rate the parent sustained from the ranks' "ready" to the last flushed file
    rate = total / (t1 - min(w.ready_at.values())) * 60.0
    st = w.parent_stats
    print(f"parent ingest: {total} games ({sum(w.game_lens)} rows) in {t1 - ready:.1f} s after ready = {rate:.0f} games/min; "
          f"parent cpu {st['cpu_s']} s, deepest backlog {st['queue_depth_max']} messages, tail after the last wave "
          f"{t1 - last_wave_sent:.1f} s")
    assert st["queue_depth_max"] <= 3 * ranks                  # per rank at most: "ready" + a wave + "done" (or the next wave)
    # the burst must be absorbed before the wave after next would arrive (on a quiet host it takes ~0.5 of a period: the
    # figure is printed; this VM's CPU share moves by 2x from run to run, so the default run only bounds it), and the long
    # soak must sustain the eight-GPU rate
    assert t1 - last_wave_sent < 2.0 * period_s
    if waves >= 5:
        assert rate >= 8 * 4700 and t1 - last_wave_sent < period_s
    # files: every one exactly games_per_file games, every id once, the rows of each game intact
    assert len(w.files) == total // 256 and all(os.path.exists(f) for f in w.files)
    seen = []
    for f in w.files:
        with np.load(f) as z:
            gid = z["game_id"]
            assert len(gid) == 256 and int(z["game_ptr"][-1]) == 256 * 54
            seen.append(gid)
            if f is w.files[0] or f is w.files[-1]:            # the id smuggled into the features matches row for row
                ids_in_rows = (z["feat"][:, 0] >> np.uint64(40)).astype(np.int64)
                assert np.array_equal(ids_in_rows, np.repeat(gid, 54))
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(total))
