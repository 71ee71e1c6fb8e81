"""Net-vs-net match on one GPU (woker/evaluation.py): `arena.Arena` plays --pairs pairs of games between two networks --
two checkpoints ({"state_dict": ...}, as self_play.py loads them) or two seeded initialisations -- and prints the
ArenaResult and one JSON line.

--bench: network A against a second InferenceNet built from the same weights, and, in the same process, a
SelfPlay(keep_records=False) of the same games, simulations and noise setting; both games-per-minute figures and the rows
each network evaluated go to profiles/arena_games_per_min.md.  The towers follow the rows they evaluate, the stem and the
heads of both networks run over the full batch: the ratio to self-play is what the second network costs.

--sims-b N: the sides search unequally, A with --sims and B with N simulations per move (Arena(sims_b=N)).  --same-weights
builds B from A's weights: the match then measures what the extra simulations are worth with that network.  --append FILE
adds the result as a section to a profile file.

--gumbel-a / --gumbel-b: that side searches with the Gumbel root (Arena(gumbel_a=, gumbel_b=); m = 16, c_visit = 50,
c_scale = 1).  --solver-a / --solver-b: that side searches with proven wins and losses below the root
(Arena(solver_a=, solver_b=)); not together with a Gumbel side."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hive_alphazero_amd import mcts                                   # noqa: E402
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet       # noqa: E402
from hive_alphazero_amd.arena import Arena                            # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "auto": None}


def load_net(checkpoint, seed):
    torch.manual_seed(seed)
    net = ChessNet()
    if checkpoint:
        net.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True)["state_dict"])
    return net.cuda().eval()


def play(arena):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = arena.run()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def bench(args, net_a, dtype):
    A, A2 = InferenceNet(net_a, dtype=dtype), InferenceNet(net_a, dtype=dtype)
    games = 2 * args.pairs
    inflight = min(args.games_in_flight, games)
    out = {}
    for label in ("warm-up", "timed"):                                  # the first run captures the graphs of every batch size
        ar = Arena(A, A2, pairs=args.pairs, sims=args.sims, slots=args.slots, games_in_flight=inflight, seed=args.seed,
                   opening_turns=args.opening_turns, noise_eps=args.noise_eps, keep_moves=False)
        res, t_arena = play(ar)
        rows, launched, illegal = ar.rows_evaluated(), ar.search.evals_launched, ar.illegal_count()
        ar.close()
        sp = mcts.SelfPlay(inflight, args.sims, A, slots=args.slots, seed=args.seed, keep_records=False, game_ids=range(games),
                           search_options={"noise_eps": args.noise_eps})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while sp.running():
            sp.play_ply()
        torch.cuda.synchronize()
        t_sp = time.perf_counter() - t0
        sp_rows, sp_launched, sp_games = int(sp.search.evals_run.item()), sp.search.evals_launched, sp.finished
        illegal += sp.env.illegal_count()
        sp.close()
        out = {"arena_games_per_min": 60.0 * res.games / t_arena, "selfplay_games_per_min": 60.0 * sp_games / t_sp,
               "arena_seconds": t_arena, "selfplay_seconds": t_sp, "games": res.games, "selfplay_games": sp_games,
               "rows_a": rows[0], "rows_b": rows[1], "arena_rows_launched": launched, "selfplay_rows": sp_rows,
               "selfplay_rows_launched": sp_launched, "illegal": illegal, "result": res.as_dict()}
        print(label, json.dumps(out), flush=True)
    assert out["illegal"] == 0 and out["games"] == out["selfplay_games"] == games
    ratio = out["arena_games_per_min"] / out["selfplay_games_per_min"]
    out["arena_over_selfplay"] = ratio
    path = os.path.join(ROOT, "profiles", "arena_games_per_min.md")
    with open(path, "w") as f:
        f.write("# Arena beside self-play: games per minute on one MI355X\n\n"
                f"`python tools/arena.py --bench --pairs {args.pairs} --sims {args.sims} --slots {args.slots} "
                f"--games-in-flight {args.games_in_flight} --noise-eps {args.noise_eps} --dtype {args.dtype}` "
                "(second run of the process, graphs captured by the first).\n\n"
                "Network A plays a second `InferenceNet` built from the same weights; `SelfPlay(keep_records=False)` plays the same\n"
                "number of games with the same simulations, slots and root-noise setting.  The arena's first "
                f"{args.opening_turns} turns are uniformly random openings without a search; self-play searches every ply.\n\n"
                "| | games | seconds | games / min | rows through a tower | rows launched |\n|---|---|---|---|---|---|\n"
                f"| arena (A vs A2) | {out['games']} | {out['arena_seconds']:.2f} | {out['arena_games_per_min']:.0f} | "
                f"A {out['rows_a']} + B {out['rows_b']} = {out['rows_a'] + out['rows_b']} | {out['arena_rows_launched']} per network |\n"
                f"| self-play (A) | {out['selfplay_games']} | {out['selfplay_seconds']:.2f} | {out['selfplay_games_per_min']:.0f} | "
                f"{out['selfplay_rows']} | {out['selfplay_rows_launched']} |\n\n"
                f"Arena / self-play games per minute: **{ratio:.2f}**.  Every launched row passes the stem and the heads of BOTH "
                "networks in the arena; only the towers follow the rows flagged for their network.\n\n"
                f"Match result (equal weights): {res!r}\n")
    print(json.dumps(out))
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoints", nargs="*", help="checkpoint of A, checkpoint of B (omit for seeded initialisations)")
    ap.add_argument("--seed-a", type=int, default=0)
    ap.add_argument("--seed-b", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--slots", type=int, default=1)
    ap.add_argument("--games-in-flight", type=int, default=1024)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--opening-turns", type=int, default=4)
    ap.add_argument("--noise-eps", type=float, default=0.0)
    ap.add_argument("--min-score", type=float, default=0.55)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--sims-b", type=int, default=None, help="simulations per move of B (default: --sims, equal sides)")
    ap.add_argument("--same-weights", action="store_true", help="B is a second InferenceNet of A's weights")
    ap.add_argument("--gumbel-a", action="store_true", help="A searches with the Gumbel root (sequential halving)")
    ap.add_argument("--gumbel-b", action="store_true", help="B searches with the Gumbel root")
    ap.add_argument("--gumbel-interior-a", action="store_true",
                    help="A's Gumbel search also selects below the root by the Gumbel rule (needs --gumbel-a)")
    ap.add_argument("--gumbel-interior-b", action="store_true", help="the same for B (needs --gumbel-b)")
    ap.add_argument("--solver-a", action="store_true", help="A searches with proven wins and losses below the root")
    ap.add_argument("--solver-b", action="store_true", help="the same for B")
    ap.add_argument("--append", default=None, metavar="FILE", help="append the result to this profile file")
    args = ap.parse_args()
    if len(args.checkpoints) not in (0, 2):
        ap.error("give two checkpoints, or none and --seed-a / --seed-b")
    if (args.gumbel_interior_a and not args.gumbel_a) or (args.gumbel_interior_b and not args.gumbel_b):
        ap.error("--gumbel-interior-a / -b need --gumbel-a / -b")
    ck = args.checkpoints or [None, None]
    net_a = load_net(ck[0], args.seed_a)
    if args.bench:
        return bench(args, net_a, DTYPES[args.dtype])
    net_b = net_a if args.same_weights else load_net(ck[1], args.seed_b)
    A, B = InferenceNet(net_a, dtype=DTYPES[args.dtype]), InferenceNet(net_b, dtype=DTYPES[args.dtype])
    ar = Arena(A, B, pairs=args.pairs, sims=args.sims, slots=args.slots, games_in_flight=args.games_in_flight, seed=args.seed,
               opening_turns=args.opening_turns, noise_eps=args.noise_eps, keep_moves=False, sims_b=args.sims_b,
               gumbel_a=args.gumbel_a or None, gumbel_b=args.gumbel_b or None, gumbel_interior_a=args.gumbel_interior_a,
               gumbel_interior_b=args.gumbel_interior_b, solver_a=args.solver_a, solver_b=args.solver_b)
    res, seconds = play(ar)
    rows = ar.rows_evaluated()
    assert ar.illegal_count() == 0
    ar.close()
    print(res)
    d = res.as_dict()
    d.update(passes=res.passes(args.min_score), passes_ci=res.passes_ci(), seconds=seconds,
             games_per_min=60.0 * res.games / seconds, rows_a=rows[0], rows_b=rows[1], sims=args.sims, seed=args.seed,
             sims_b=args.sims_b if args.sims_b is not None else args.sims, gumbel_a=args.gumbel_a, gumbel_b=args.gumbel_b,
             gumbel_interior_a=args.gumbel_interior_a, gumbel_interior_b=args.gumbel_interior_b, solver_a=args.solver_a,
             solver_b=args.solver_b)
    print(json.dumps(d))
    if args.append:
        with open(args.append, "a") as f:
            f.write(f"\n## Arena: {args.sims} against {d['sims_b']} simulations"
                    + (", one set of weights" if args.same_weights else "")
                    + (", Gumbel root for " + " and ".join(n for n, on in (("A", args.gumbel_a), ("B", args.gumbel_b)) if on)
                       if args.gumbel_a or args.gumbel_b else "")
                    + (", also below the root for " + " and ".join(n for n, on in (("A", args.gumbel_interior_a),
                                                                                  ("B", args.gumbel_interior_b)) if on)
                       if args.gumbel_interior_a or args.gumbel_interior_b else "")
                    + (", proven wins and losses for " + " and ".join(n for n, on in (("A", args.solver_a), ("B", args.solver_b)) if on)
                       if args.solver_a or args.solver_b else "") + "\n\n"
                    f"`python tools/arena.py --pairs {args.pairs} --sims {args.sims} --sims-b {d['sims_b']} --seed {args.seed} "
                    f"--noise-eps {args.noise_eps} --dtype {args.dtype}" + (" --same-weights" if args.same_weights else "")
                    + (" --gumbel-a" if args.gumbel_a else "") + (" --gumbel-b" if args.gumbel_b else "")
                    + (" --gumbel-interior-a" if args.gumbel_interior_a else "")
                    + (" --gumbel-interior-b" if args.gumbel_interior_b else "")
                    + (" --solver-a" if args.solver_a else "") + (" --solver-b" if args.solver_b else "") + "`\n\n"
                    f"A searches {args.sims} simulations per move, B {d['sims_b']}.  {res!r}\n\n"
                    f"Score of A {res.score:.3f}, 95 % interval [{res.score_ci95[0]:.3f}, {res.score_ci95[1]:.3f}] over "
                    f"{len(res.pair_scores)} pairs ({res.games} games in {seconds:.1f} s); rows through a tower: A {rows[0]}, "
                    f"B {rows[1]}.\n")
        print("appended to", args.append)


if __name__ == "__main__":
    main()
