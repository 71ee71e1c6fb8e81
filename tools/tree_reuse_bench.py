"""Whole-game self-play (1024 games x 50 sims from the opening, engine only, fp16 net) with the trees emptied on every move
(keep_tree off: the reference, and what every other tool runs) and kept across plies (keep_tree on), interleaved in ONE
process on one box.  Timed rounds report games/min; one further instrumented round per form (a device synchronise and a
statistics read per ply, so its games/min are not reported) gives the time of the root launch (hive_search_set_roots /
hive_search_advance_roots, device events), the kept nodes, the carried visits, the refused carries and the leaf histogram."""
import argparse, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hive_alphazero_amd import mcts
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=1024)
ap.add_argument("--sims", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-nodes", type=int, default=0, help="node pool per game with keep_tree (0 = TreeSearch's default)")
args = ap.parse_args()
G, SIMS = args.games, args.sims
torch.manual_seed(0)
inf = InferenceNet(ChessNet().cuda().eval(), dtype=torch.float16)
keep_opt = {"keep_tree": True}
if args.max_nodes:
    keep_opt["max_nodes"] = args.max_nodes
forms = (("keep_tree off", {}), ("keep_tree on", keep_opt))
NODE_BYTES = 64 + 384 + 4 + 4 + 1 + 4 + 256 * (2 + 4 + 4 + 4 + 4)


class TimedRoots:
    """The library with device events around the root launch of every search."""

    def __init__(self, lib):
        self._lib, self.pairs = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("hive_search_set_roots", "hive_search_advance_roots"):
            return fn

        def timed(*a):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = fn(*a)
            t1.record()
            self.pairs.append((t0, t1))
            return rc
        return timed


def play(opt, instrument):
    sp = mcts.SelfPlay(G, SIMS, inf, seed=1234, keep_records=False, game_ids=range(G), search_options=opt)
    timer = None
    if instrument:
        timer = sp.search.L = TimedRoots(sp.search.L)
    per_ply = []
    torch.cuda.synchronize(); t0 = time.perf_counter(); plies = 0
    while True:
        running = sp.active.clone() if instrument else None
        sp.play_ply(); plies += 1
        if instrument and sp.search.keep_tree:
            kept, visits, refused = sp.search.carry_stats()
            on = (running != 0) & (sp.search.action != -2)
            per_ply.append((int(on.sum()), int(kept[on].sum()), int(kept.max()), int(visits[on].sum()), int((kept[on] > 0).sum()),
                            int(refused.sum())))
        if sp.running() == 0 or plies > 60:
            break
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    out = {"games_per_min": sp.finished / el * 60, "seconds": el, "plies": plies, "finished": sp.finished,
           "results": (sp.white_wins, sp.black_wins, sp.draws), "mean_len": sp.mean_game_length(),
           "rows": int(sp.search.evals_run.item()), "launched": sp.search.evals_launched, "hist": sp.leaf_histogram(),
           "max_nodes": sp.search.max_nodes, "per_ply": per_ply}
    if timer is not None:
        ms = sorted(a.elapsed_time(b) for a, b in timer.pairs[1:])          # (the first advance allocates the second pool)
        out["root_launch_us"] = (1e3 * ms[len(ms) // 2], 1e3 * ms[0], 1e3 * ms[-1], len(ms))
    sp.close()
    return out


warm = mcts.SelfPlay(G, SIMS, inf, seed=1234, keep_records=False, search_options=keep_opt)
warm.play_ply(); warm.play_ply(); torch.cuda.synchronize(); warm.close()
for rnd in range(args.rounds):
    for name, opt in forms:
        r = play(opt, False)
        print(f"round {rnd}  {name:14s} {r['games_per_min']:8.1f} games/min  {r['seconds']:6.2f} s  {r['plies']} plies  rows evaluated "
              f"{r['rows']} of {r['launched']}  mean game length {r['mean_len']:.1f}  results W{r['results'][0]} B{r['results'][1]} "
              f"D{r['results'][2]}", flush=True)
for name, opt in forms:
    r = play(opt, True)
    med, lo, hi, n = r["root_launch_us"]
    pool = G * r["max_nodes"] * NODE_BYTES * (2 if opt.get("keep_tree") else 1) / 2 ** 30
    print(f"instrumented  {name:14s} root launch median {med:.1f} us (min {lo:.1f}, max {hi:.1f}, {n} plies)  max_nodes "
          f"{r['max_nodes']}  node pool {pool:.2f} GiB  leaves {r['hist']}", flush=True)
    if r["per_ply"]:
        searched = sum(p[0] for p in r["per_ply"][1:])
        kept_sum = sum(p[1] for p in r["per_ply"][1:])
        carried = sum(p[4] for p in r["per_ply"][1:])
        print(f"              searches after the first ply {searched}: carried {carried} ({100.0 * carried / searched:.1f} %), refused "
              f"{r['per_ply'][-1][5]} ({100.0 * r['per_ply'][-1][5] / searched:.2f} %), kept nodes mean {kept_sum / searched:.1f} max "
              f"{max(p[2] for p in r['per_ply'])}, carried visits / sims mean "
              f"{sum(p[3] for p in r['per_ply'][1:]) / searched / SIMS:.3f}, bytes moved per ply (mean kept nodes x {NODE_BYTES} B "
              f"upper bound x {G} games) {kept_sum / searched * NODE_BYTES * G / 2 ** 20:.1f} MiB", flush=True)
