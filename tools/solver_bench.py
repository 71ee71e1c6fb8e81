"""Proven wins and losses below the root beside the plain search: 1024 whole games from the opening, engine only, in four forms
interleaved in ONE process for two rounds -- PUCT at 50 simulations in lock step and the playout cap 50 / 10 / 0.25 rolling,
each with the option off and on -- the same network, seed and game ids as tools/gumbel_bench.py.  The games of the forms are
different games: there is no threshold, the figures are a record.  Per form: games/min, moves/s (game lengths differ), mean
length, decisive share, leaf rows launched and evaluated, and the four counters of hive_search_solver_stats.  Writes the second
round's table and both rounds' games/min into the section "## Option off and on: four forms" of profiles/solver.md --
replaced if it is there, appended if not; every other section of the file is kept as it is."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hive_alphazero_amd import mcts
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
torch.manual_seed(0)
inf = InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16)
G, FULL, FAST, P = 1024, 50, 10, 0.25
CAP = {"full": FULL, "fast": FAST, "p_full": P, "quiet_fast": True}
ON = {"solver": True}
forms = (("PUCT 50", None, None, None), ("PUCT 50 + solver", None, None, ON),
         (f"PUCT cap {FULL}/{FAST}/{P} rolling", CAP, True, None), (f"PUCT cap {FULL}/{FAST}/{P} rolling + solver", CAP, True, ON))
warm = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False); warm.play_ply(); torch.cuda.synchronize(); warm.close()


def play(name, cap, rolling, options):
    sp = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False, game_ids=range(G), playout_cap=cap, rolling=rolling,
                       search_options=options)
    moves = torch.zeros((1,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize(); t0 = time.perf_counter(); calls = 0
    while True:
        sp.play_ply(); calls += 1
        moves += (sp.search.action != -2).sum()
        if sp.running() == 0 or calls > 4000: break
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    stats = sp.search.solver_stats().sum(0).cpu().tolist()
    row = {"name": name, "games": sp.finished, "s": el, "gpm": sp.finished / el * 60, "mps": int(moves.item()) / el,
           "length": sp.mean_game_length(), "decisive": (sp.white_wins + sp.black_wins) / max(sp.finished, 1),
           "results": f"W{sp.white_wins} B{sp.black_wins} D{sp.draws}", "launched": sp.search.evals_launched,
           "evaluated": int(sp.search.evals_run.item()), "stats": stats, "sims": sum(sp.leaf_histogram().values()),
           "illegal": sp.env.illegal_count()}
    print(f"{name:40s} {row['gpm']:8.1f} games/min {row['mps']:8.0f} moves/s {el:6.2f} s  length {row['length']:.2f}  decisive "
          f"{row['decisive']:.3f} ({row['results']})  rows launched {row['launched']} evaluated {row['evaluated']}  "
          f"simulations {row['sims']}  stops / wins / losses / answers {stats}", flush=True)
    assert row["illegal"] == 0 and row["games"] == G
    sp.close()
    return row


rounds = [[play(*f) for f in forms] for _ in range(2)]
table = rounds[1]
path = os.path.join(ROOT, "profiles", "solver.md")
HEAD = "\n## Option off and on: four forms\n"
old = open(path).read() if os.path.exists(path) else "# Proven wins and losses below the root on one MI355X\n"
before, after = old, ""
if HEAD in old:
    before, rest = old.split(HEAD, 1)
    after = rest[rest.index("\n## "):] if "\n## " in rest else ""
with open(path, "w") as f:
    f.write(before.rstrip("\n") + "\n" + HEAD + "\n"
            "`python tools/solver_bench.py`: 1024 whole games from the opening, engine only (`keep_records=False`), bf16 "
            "`InferenceNet` with random weights, seed 1234, game ids 0..1023; the four forms interleaved in one process for two "
            "rounds, second round of the process.  \"+ solver\" is `search_options={\"solver\": True}`.  The forms play different "
            "games: games per minute is not comparable across rows, moves per second is the figure that does not depend on the "
            "game lengths, and no threshold applies.  Rows launched are the leaf rows handed to the evaluator, rows evaluated "
            "those a tower ran on (unread rows and equal leaves are skipped).  The counters are sums over the games: descents "
            "ended at a proven node, nodes that became proven wins, proven losses, answers taken from a proof.\n\n"
            "| | games | seconds | games / min | moves / s | mean length | decisive share | results | rows launched | rows evaluated | "
            "simulations | ended at a proof | proven wins | proven losses | answers from a proof |\n"
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for t in table:
        f.write(f"| {t['name']} | {t['games']} | {t['s']:.2f} | {t['gpm']:.0f} | {t['mps']:.0f} | {t['length']:.2f} | "
                f"{t['decisive']:.3f} | {t['results']} | {t['launched']} | {t['evaluated']} | {t['sims']} | "
                + " | ".join(str(int(x)) for x in t["stats"]) + " |\n")
    f.write("\nGames per minute in both rounds of the process: " +
            "; ".join(f"{a['name']} {a['gpm']:.0f}, {b['gpm']:.0f}" for a, b in zip(*rounds)) + ".\n")
    f.write(after)
print("wrote", path)
