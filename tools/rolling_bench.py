"""Whole-game self-play (1024 games from the opening, engine only) in three forms -- plain (50 simulations on every ply),
playout cap in lock step (50 / 10 simulations, a quarter of the plies full) and the same cap rolling (every game moves when
its own search is done) -- interleaved in ONE process for two rounds, the same network, seed and game ids as
tools/playout_cap_bench.py.  The two capped forms play the same games, bit for bit: asserted.  Then both capped forms with
game ids that never run out (every finished game is replaced), timed over a window: the batch above drains as its games end,
a producer's does not.  Writes the second round's table, both rounds' games/min, the refilled window and the host memory of
the record log to profiles/rolling_selfplay.md."""
import itertools, os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hive_alphazero_amd import mcts
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
torch.manual_seed(0)
inf = InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16)
G, FULL, FAST, P = 1024, 50, 10, 0.25
CAP = {"full": FULL, "fast": FAST, "p_full": P, "quiet_fast": True}
forms = (("plain 50", None, None), (f"cap {FULL}/{FAST}/{P} lock step", CAP, None), (f"cap {FULL}/{FAST}/{P} rolling", CAP, True))
warm = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False); warm.play_ply(); torch.cuda.synchronize(); warm.close()


def play(name, cap, rolling):
    sp = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False, game_ids=range(G), playout_cap=cap, rolling=rolling)
    slots = sp.search.slots
    torch.cuda.synchronize(); t0 = time.perf_counter(); calls = 0
    full_count = torch.zeros((), dtype=torch.int64, device="cuda")
    while True:
        sp.play_ply(); calls += 1
        # training rows = searched plies drawn full (every searched ply without a cap); counted on the device, read once
        full_count += ((sp.search.action != -2) & ((sp.full != 0) if cap else True)).sum()
        if sp.running() == 0 or calls > 400: break
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    launched = sp.search.evals_launched
    # lock step: a ply is 1 + ceil((sims - 1) / slots) rounds; rolling: a turn-over is `quantum` rounds
    rounds = calls * (sp.rolling["quantum"] if rolling else mcts.rolling_quantum(FULL, slots))
    row = {"name": name, "games": sp.finished, "s": el, "gpm": sp.finished / el * 60, "rounds": rounds, "launched": launched,
           "evaluated": int(sp.search.evals_run.item()), "sims": sum(sp.leaf_histogram().values()),
           "train": int(full_count.item()), "results": f"W{sp.white_wins} B{sp.black_wins} D{sp.draws}",
           "length": sp.mean_game_length(), "illegal": sp.env.illegal_count()}
    row["live"] = row["sims"] / launched
    row["train_pm"] = row["train"] / el * 60
    print(f"{name:26s} {row['gpm']:8.1f} games/min  {el:6.2f} s  rounds {rounds}  rows evaluated {row['evaluated']} of {launched} "
          f"launched  simulations {row['sims']} (live share {row['live']:.3f})  training rows {row['train']} "
          f"({row['train_pm']:.0f}/min)  results {row['results']}  mean length {row['length']:.2f}", flush=True)
    assert row["illegal"] == 0 and row["games"] == G
    sp.close()
    return row


def refilled(name, rolling, warm_rounds, timed_rounds):
    """The capped engine with ids that never run out: `warm_rounds` rounds untimed, then a window of `timed_rounds`."""
    sp = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False, game_ids=itertools.count(), playout_cap=CAP, rolling=rolling)
    per_call = sp.rolling["quantum"] if rolling else mcts.rolling_quantum(FULL, sp.search.slots)
    moved = torch.zeros((), dtype=torch.int64, device="cuda")
    for _ in range(-(-warm_rounds // per_call)):
        sp.play_ply()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    sims0, launched0, finished0 = sum(sp.leaf_histogram().values()), sp.search.evals_launched, sp.finished
    calls = -(-timed_rounds // per_call)
    for _ in range(calls):
        sp.play_ply()
        moved += (sp.search.action != -2).sum()
    sp.retire_finished()
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    sims, launched = sum(sp.leaf_histogram().values()) - sims0, sp.search.evals_launched - launched0
    row = {"name": name, "rounds": calls * per_call, "s": el, "moves": int(moved.item()), "games": sp.finished - finished0,
           "sims": sims, "live": sims / launched}
    print(f"refilled {name:12s} {row['rounds']} rounds in {el:.2f} s: {row['moves']} moves ({row['moves'] / el:.0f}/s), "
          f"{row['games']} games finished ({row['games'] / el * 60:.0f}/min), simulations {sims} (live share {row['live']:.3f})", flush=True)
    assert sp.env.illegal_count() == 0 and sp.running() == G
    sp.close()
    return row


def log_bytes(rolling):
    """(peak host memory of the record log, entries at the peak, seconds of the run): records.PlyLog -- every array of every
    entry a running game still needs, the staging sets included -- over a capped run of the 1024 games that keeps its records."""
    torch.cuda.synchronize(); t0 = time.perf_counter()
    sp = mcts.SelfPlay(G, FULL, inf, seed=1234, game_ids=range(G), packed_records=True, max_finished_kept=2 * G, playout_cap=CAP,
                       rolling=rolling)
    peak = entries = calls = 0
    while sp.running() and calls < 400:
        sp.play_ply(); calls += 1
        sp.drain_finished_packed()
        size = 0
        for e in sp._plylog.entries:
            size += sum(v.nbytes for v in e.values() if hasattr(v, "nbytes"))
            size += sum(a.nbytes for a in e.get("csr", ()))
        if size > peak:
            peak, entries = size, len(sp._plylog.entries)
    torch.cuda.synchronize()
    assert sp.finished == G and sp.dropped_games == 0
    sp.close()
    return peak, entries, time.perf_counter() - t0


rounds = [[play(*f) for f in forms] for _ in range(2)]
table = rounds[1]
plain, lock, roll = table
for key in ("results", "length", "sims", "illegal", "games"):
    assert lock[key] == roll[key], (key, lock[key], roll[key])       # the games are the same bits
spread = abs(rounds[0][1]["gpm"] - rounds[1][1]["gpm"])
faster = roll["gpm"] - lock["gpm"] > spread
# lock step: games refilled together stay together, one cycle is 54-55 plies of 50 rounds; rolling: one mean game (about
# 1,100 rounds) untimed first, so that the window sees slots refilled at their own times
window = [refilled("lock step", None, 50, 2750), refilled("rolling", True, 1500, 2750)]
mem = {name: log_bytes(r) for name, r in (("lock step", None), ("rolling", True))}
path = os.path.join(ROOT, "profiles", "rolling_selfplay.md")
# sections below this heading are measured otherwise (bench.py on two trees, a kernel trace) and written by hand: kept
KEEP = "\n## The option off"
kept = ""
if os.path.exists(path):
    old = open(path).read()
    kept = old[old.index(KEEP):] if KEEP in old else ""
with open(path, "w") as f:
    f.write("# Rolling self-play beside the lock-step engine on one MI355X\n\n"
            "`python tools/rolling_bench.py`: 1024 whole games from the opening, engine only (`keep_records=False`), bf16 "
            "`InferenceNet` with random weights, seed 1234, game ids 0..1023; the three forms interleaved in one process for two "
            "rounds, second round of the process.  A round of the search = one leaf batch (select, leaves, network, backup); "
            "live share = simulations / leaf rows launched.\n\n"
            "| | games | seconds | games / min | rounds | leaf rows launched | leaf rows evaluated | simulations | live share | "
            "training rows | training rows / min | results | mean length |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for t in table:
        f.write(f"| {t['name']} | {t['games']} | {t['s']:.2f} | {t['gpm']:.0f} | {t['rounds']} | {t['launched']} | {t['evaluated']} | "
                f"{t['sims']} | {t['live']:.3f} | {t['train']} | {t['train_pm']:.0f} | {t['results']} | {t['length']:.2f} |\n")
    f.write("\nGames per minute in both rounds of the process: " +
            "; ".join(f"{a['name']} {a['gpm']:.0f}, {b['gpm']:.0f}" for a, b in zip(*rounds)) + ".\n\n")
    f.write(f"Capped rolling / capped lock step: games per minute **{roll['gpm'] / lock['gpm']:.2f}** ({roll['gpm']:.0f} against "
            f"{lock['gpm']:.0f}; the lock-step form's two rounds lie {spread:.0f} games/min apart: rolling is "
            f"{'faster by more than that spread' if faster else 'NOT faster by more than that spread'}), rounds "
            f"{roll['rounds'] / lock['rounds']:.2f}, rows launched {roll['launched'] / lock['launched']:.2f}.  Against the plain "
            f"engine: lock step {lock['gpm'] / plain['gpm']:.2f}, rolling {roll['gpm'] / plain['gpm']:.2f} (simulations "
            f"{lock['sims'] / plain['sims']:.2f}).\n"
            f"Both capped forms: results {lock['results']}, mean length {lock['length']:.2f} plies, {lock['sims']} simulations, no "
            "move refused by the env -- the same games (asserted by the tool).\n"
            f"Equal-leaf sharing, rows evaluated / simulations: plain {plain['evaluated'] / plain['sims']:.3f}, lock step "
            f"{lock['evaluated'] / lock['sims']:.3f}, rolling {roll['evaluated'] / roll['sims']:.3f} -- games that left the common "
            "clock ask about the same position in different rounds.\n\n"
            "## Ids that never run out\n\n"
            "The 1024 games above are all there is: slots go idle as games end, and the last rounds serve the few games that "
            "drew the most full plies (the lock-step form ends every game within a ply or two of ply 54 instead).  A producer "
            "replaces every finished game.  Both capped forms with `game_ids=itertools.count()`, a window of 2750 rounds after "
            "50 (lock step: one cycle of its games) and 1500 (rolling: past one mean game, so slots are refilled at their own "
            "times) untimed rounds; a move = one ply of one game:\n\n"
            "| | rounds | seconds | moves | moves / s | games finished | games / min | simulations | live share |\n"
            "|---|---|---|---|---|---|---|---|---|\n" +
            "".join(f"| {w['name']} | {w['rounds']} | {w['s']:.2f} | {w['moves']} | {w['moves'] / w['s']:.0f} | {w['games']} | "
                    f"{w['games'] / w['s'] * 60:.0f} | {w['sims']} | {w['live']:.3f} |\n" for w in window) +
            f"\nRolling / lock step: moves per second **{(window[1]['moves'] / window[1]['s']) / (window[0]['moves'] / window[0]['s']):.2f}**.\n\n"
            "## Host memory of the record log\n\n"
            "A capped run that keeps its records (`packed_records=True`, drained after every call): peak bytes of "
            "`records.PlyLog`'s entries, staging sets and sparse policies included.  A log entry is a whole-batch copy per "
            "`play_ply()` call; rolling makes one call per turn-over, so a game spans more entries.\n\n"
            "Seconds: the whole run with its records (engine built, 1024 games played, packed and drained).\n\n"
            "| | peak MB | entries at the peak | seconds |\n|---|---|---|---|\n")
    for name, (peak, entries, seconds) in mem.items():
        f.write(f"| {name} | {peak / 1e6:.0f} | {entries} | {seconds:.2f} |\n")
    f.write(kept)
print("wrote", path)
