"""Whole-game self-play (1024 games from the opening, engine only) plain -- 50 simulations on every ply -- and with playout-cap
randomisation (50 / 10 simulations, a quarter of the plies full), interleaved in ONE process on one box (boxes differ by
2-5 %), the same game ids in both: games/min, leaf rows launched and evaluated, training rows/min.  Writes the second
round's table to profiles/playout_cap.md."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hive_alphazero_amd import mcts
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet
torch.manual_seed(0)
inf = InferenceNet(ChessNet().cuda().eval(), dtype=torch.bfloat16)
G, FULL, FAST, P = 1024, 50, 10, 0.25
forms = (("plain 50", None), (f"cap {FULL}/{FAST}/{P}", {"full": FULL, "fast": FAST, "p_full": P, "quiet_fast": True}))
warm = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False); warm.play_ply(); torch.cuda.synchronize(); warm.close()
table = []
for rnd in range(2):
    table = []
    for name, cap in forms:
        sp = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False, game_ids=range(G), playout_cap=cap)
        torch.cuda.synchronize(); t0 = time.perf_counter(); plies = full_rows = 0
        full_count = torch.zeros((), dtype=torch.int64, device="cuda")
        while True:
            sp.play_ply(); plies += 1
            # training rows = searched plies drawn full (every searched ply without a cap); counted on the device, read once
            full_count += ((sp.search.action != -2) & ((sp.full != 0) if cap else True)).sum()
            if sp.running() == 0 or plies > 60: break
        torch.cuda.synchronize(); el = time.perf_counter() - t0
        full_rows = int(full_count.item())
        rows, launched = int(sp.search.evals_run.item()), sp.search.evals_launched
        sims_run = sum(sp.leaf_histogram().values())
        line = (name, sp.finished, el, sp.finished / el * 60, launched, rows, sims_run, full_rows, full_rows / el * 60,
                f"W{sp.white_wins} B{sp.black_wins} D{sp.draws}", sp.mean_game_length())
        table.append(line)
        print(f"{name:18s} {line[3]:8.1f} games/min  {el:6.2f} s  rows evaluated {rows} of {launched} launched  simulations {sims_run}  "
              f"training rows {full_rows} ({line[8]:.0f}/min)  results {line[9]}  mean length {line[10]:.1f}", flush=True)
        assert sp.env.illegal_count() == 0
        sp.close()
plain, capped = table
path = os.path.join(ROOT, "profiles", "playout_cap.md")
with open(path, "w") as f:
    f.write("# Playout-cap self-play beside the plain engine on one MI355X\n\n"
            "`python tools/playout_cap_bench.py`: 1024 whole games from the opening, engine only (`keep_records=False`), bf16 "
            "`InferenceNet` with random weights, the same game ids and seed; plain and capped runs interleaved in one process, "
            "second round of the process.\n\n"
            "| | games | seconds | games / min | leaf rows launched | leaf rows evaluated | simulations | training rows | training rows / min |\n"
            "|---|---|---|---|---|---|---|---|---|\n")
    for t in table:
        f.write(f"| {t[0]} | {t[1]} | {t[2]:.2f} | {t[3]:.0f} | {t[4]} | {t[5]} | {t[6]} | {t[7]} | {t[8]:.0f} |\n")
    f.write(f"\nCapped / plain: games per minute **{capped[3] / plain[3]:.2f}**, rows evaluated {capped[5] / plain[5]:.2f} "
            f"(simulations {capped[6] / plain[6]:.2f}; the arithmetic says ({P} x {FULL} + {1 - P} x {FAST}) / {FULL} = "
            f"{(P * FULL + (1 - P) * FAST) / FULL:.2f}), rows launched {capped[4] / plain[4]:.2f}, training rows per minute "
            f"{capped[8] / plain[8]:.2f}.  The batch still runs {FULL} rounds per ply: a dropped-out game leaves a hole that the "
            "stem, the heads and the planes writer still pass over, and every round keeps its fixed launch cost; only the tower "
            "follows the rows evaluated.\n"
            f"Results plain {plain[9]}, mean length {plain[10]:.1f} plies; capped {capped[9]}, mean length {capped[10]:.1f} plies.\n")
print("wrote", path)
