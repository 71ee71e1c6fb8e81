"""The Gumbel root beside the PUCT root: 1024 whole games from the opening, engine only, in six forms interleaved in ONE
process for two rounds -- plain PUCT, Gumbel (root only) and full Gumbel (the rule below the root too) at 50 simulations in
lock step, and the playout cap 50 / 10 / 0.25 rolling in all three -- the same network, seed and game ids as
tools/rolling_bench.py.  The games of the forms are different games: there is no threshold, the figures are a record.  Per form: games/min, moves/s (game lengths differ), mean length, decisive
share, and over the training targets (the policy rows of the searched plies; under a cap the full plies) the mean entropy and
support size, plus how often a Gumbel root selection found no edge at the scheduled visit count.  Writes the second round's
table and both rounds' games/min into the section "## Root-only and full Gumbel: six forms" of profiles/gumbel_root.md --
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
ROOT_ONLY, FULL_GUMBEL = {"gumbel": True}, {"gumbel": True, "gumbel_interior": True}
forms = (("PUCT 50", None, None, None), ("Gumbel 50", None, None, ROOT_ONLY), ("Gumbel full 50", None, None, FULL_GUMBEL),
         (f"PUCT cap {FULL}/{FAST}/{P} rolling", CAP, True, None), (f"Gumbel cap {FULL}/{FAST}/{P} rolling", CAP, True, ROOT_ONLY),
         (f"Gumbel full cap {FULL}/{FAST}/{P} rolling", CAP, True, FULL_GUMBEL))
warm = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False); warm.play_ply(); torch.cuda.synchronize(); warm.close()


def play(name, cap, rolling, gumbel):
    sp = mcts.SelfPlay(G, FULL, inf, seed=1234, keep_records=False, game_ids=range(G), playout_cap=cap, rolling=rolling,
                       search_options=gumbel)
    acc = torch.zeros((4,), dtype=torch.float64, device="cuda")         # moves, target rows, their entropy sum, support sum
    torch.cuda.synchronize(); t0 = time.perf_counter(); calls = 0
    while True:
        sp.play_ply(); calls += 1
        moved = sp.search.action != -2
        rows = moved & (sp.full != 0) if cap else moved
        pol = sp.search.policy
        ent = -(pol * torch.log(pol.clamp_min(1e-30))).sum(1)
        acc += torch.stack([moved.sum(), rows.sum(), (ent * rows).sum(), ((pol > 0).sum(1) * rows).sum()]).double()
        if sp.running() == 0 or calls > 4000: break
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    moves, rows, ent, support = acc.cpu().tolist()
    row = {"name": name, "games": sp.finished, "s": el, "gpm": sp.finished / el * 60, "mps": moves / el,
           "length": sp.mean_game_length(), "decisive": (sp.white_wins + sp.black_wins) / max(sp.finished, 1),
           "results": f"W{sp.white_wins} B{sp.black_wins} D{sp.draws}", "rows": int(rows), "entropy": ent / max(rows, 1),
           "support": support / max(rows, 1), "fallbacks": int(sp.search.gumbel_fallbacks().sum().item()),
           "sims": sum(sp.leaf_histogram().values()), "illegal": sp.env.illegal_count()}
    print(f"{name:30s} {row['gpm']:8.1f} games/min {row['mps']:8.0f} moves/s {el:6.2f} s  length {row['length']:.2f}  decisive "
          f"{row['decisive']:.3f} ({row['results']})  targets {row['rows']}: entropy {row['entropy']:.3f} nats, support "
          f"{row['support']:.1f}  fallbacks {row['fallbacks']}  simulations {row['sims']}", flush=True)
    assert row["illegal"] == 0 and row["games"] == G
    sp.close()
    return row


rounds = [[play(*f) for f in forms] for _ in range(2)]
table = rounds[1]
path = os.path.join(ROOT, "profiles", "gumbel_root.md")
HEAD = "\n## Root-only and full Gumbel: six forms\n"
old = open(path).read() if os.path.exists(path) else "# The Gumbel root beside the PUCT root on one MI355X\n"
before, after = old, ""
if HEAD in old:
    before, rest = old.split(HEAD, 1)
    after = rest[rest.index("\n## "):] if "\n## " in rest else ""
with open(path, "w") as f:
    f.write(before.rstrip("\n") + "\n" + HEAD + "\n"
            "`python tools/gumbel_bench.py`: 1024 whole games from the opening, engine only (`keep_records=False`), bf16 "
            "`InferenceNet` with random weights, seed 1234, game ids 0..1023; the six forms interleaved in one process for two "
            "rounds, second round of the process.  \"Gumbel\" is the Gumbel root over the PUCT descent (`gumbel=True`), "
            "\"Gumbel full\" adds the Gumbel rule below the root (`gumbel_interior=True`); m = 16, c_visit = 50, c_scale = 1 -- "
            "the paper's values, not tuned for this game.  The forms play different games: games per minute is not comparable "
            "across rows, moves per second is the figure that does not depend on the game lengths, and no threshold applies.  "
            "Columns as in the table at the top of this file.\n\n"
            "| | games | seconds | games / min | moves / s | mean length | decisive share | results | target rows | mean entropy | "
            "mean support | simulations | no eligible edge |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
    for t in table:
        f.write(f"| {t['name']} | {t['games']} | {t['s']:.2f} | {t['gpm']:.0f} | {t['mps']:.0f} | {t['length']:.2f} | "
                f"{t['decisive']:.3f} | {t['results']} | {t['rows']} | {t['entropy']:.3f} | {t['support']:.1f} | {t['sims']} | "
                f"{t['fallbacks']} |\n")
    f.write("\nGames per minute in both rounds of the process: " +
            "; ".join(f"{a['name']} {a['gpm']:.0f}, {b['gpm']:.0f}" for a, b in zip(*rounds)) + ".\n")
    f.write(after)
print("wrote", path)
