"""The whole AlphaZero loop of the reference on one MI355X, end to end (self_play.py -> optimize.py/train.py -> workers
reload the weights): GPU self-play with packed per-ply records -> the trainer's tensors widened ON THE GPU from the packed
features (records.dataset_tensors_gpu_packed: the same planes, policies and 0.99 ** k discounted values optimize.py:42-65
builds from the reference's JSON rows; that equivalence is what tests/test_gpu_scale.py and tests/test_host_cpu.py check)
-> Trainer steps on the same ChessNet -> InferenceNet.refresh -> next round of self-play.  Sized to run in well under a minute.

--gate PAIRS (default 0 = off): after training, the trained network plays PAIRS pairs of arena games (arena.Arena) against
the network the round started from, and the self-play evaluator is refreshed only if it passes AlphaZero's gate
(ArenaResult.passes(): score >= 0.55).

--replay ROWS (default 0 = train on the round's own rows, as above): the rounds share one replay.ReplayBuffer of ROWS rows
on the GPU; every round appends its packed batches (1.5 KB per row go up, nothing is widened ahead of time) and the 20
training steps draw their minibatches from the whole window with buf.sample(512, step=...) -- one launch per minibatch.

--playout-cap FULL,FAST,P (default off): playout-cap randomisation, mcts.SelfPlay(playout_cap=...): a ply is searched with
FULL simulations with probability P and becomes a training row, else with FAST simulations and no root noise; the round's
search then runs max(FULL, FAST) simulations and the trainer sees the rows flagged full (both routes filter them).

--rolling (default off): mcts.SelfPlay(rolling=True) -- every game moves when its own search is done instead of waiting for
the longest search of the batch; the same games, bit for bit, in fewer rounds when the plies' searches differ in length.

--gumbel (default off): the Gumbel root with sequential halving; --gumbel-interior adds the Gumbel rule below the root (it
requires --gumbel).

--solver (default off): proven wins and losses below the root, mcts.SelfPlay(search_options={"solver": True}); not with
--gumbel."""
import argparse, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hive_alphazero_amd import mcts, records
from hive_alphazero_amd.alpha_net import ChessNet, InferenceNet, Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--gate", type=int, default=0, metavar="PAIRS", help="arena pairs that gate the refresh (0 = refresh always)")
ap.add_argument("--replay", type=int, default=0, metavar="ROWS", help="train from a replay window of ROWS rows shared by the rounds (0 = off)")
ap.add_argument("--playout-cap", default=None, metavar="FULL,FAST,P", help="full / fast simulations and the share of full plies, e.g. 16,4,0.25")
ap.add_argument("--rolling", action="store_true", help="every game moves when its own search is done (same games, fewer rounds under a playout cap)")
ap.add_argument("--gumbel", action="store_true", help="Gumbel root with sequential halving; the records hold the improved policy")
ap.add_argument("--gumbel-interior", action="store_true", help="with --gumbel: the Gumbel rule also selects below the root")
ap.add_argument("--solver", action="store_true", help="proven wins and losses below the root (not with --gumbel)")
opts = ap.parse_args()
if opts.gumbel_interior and not opts.gumbel:
    ap.error("--gumbel-interior requires --gumbel")
if opts.solver and opts.gumbel:
    ap.error("--solver is not combined with --gumbel")
gate, window = opts.gate, opts.replay
cap = None
if opts.playout_cap:
    full, fast, p_full = opts.playout_cap.split(",")
    cap = {"full": int(full), "fast": int(fast), "p_full": float(p_full)}
buf = None
if window > 0:
    from hive_alphazero_amd.replay import ReplayBuffer
    buf = ReplayBuffer(window)
games, sims, rounds = 256, (max(cap["full"], cap["fast"]) if cap else 16), 2
torch.manual_seed(0)
net = ChessNet().cuda()
evaluator = InferenceNet(net)
trainer = Trainer(net)
for rnd in range(rounds):
    net.eval()
    sp = mcts.SelfPlay(games, sims, evaluator, seed=100 + rnd, game_ids=range(rnd * games, (rnd + 1) * games),
                       packed_records=True, max_finished_kept=2 * games, playout_cap=cap, rolling=opts.rolling or None,
                       search_options={"gumbel": True, "gumbel_interior": opts.gumbel_interior} if opts.gumbel
                       else ({"solver": True} if opts.solver else None))
    t0 = time.perf_counter()
    batches = []
    while sp.running() and sp.plies < (80 * sims if opts.rolling else 80):      # (rolling: plies counts turn-overs)
        sp.play_ply()
        b = sp.drain_finished_packed()
        if b is not None:
            batches.append(b)
    torch.cuda.synchronize()
    t_sp = time.perf_counter() - t0
    illegal, results = sp.env.illegal_count(), (sp.white_wins, sp.black_wins, sp.draws)
    assert sp.dropped_games == 0 and sp.unrecorded_games == 0
    sp.close()
    packed = records.concat_packed(batches)
    t0 = time.perf_counter()
    if buf is not None:
        n = sum(buf.add_packed(b) for b in batches)
    else:
        states, policies, values = records.dataset_tensors_gpu_packed(packed, dtype=torch.float32, layout="chw")
        n = states.shape[0]
    torch.cuda.synchronize()
    t_ds = time.perf_counter() - t0
    t0 = time.perf_counter()
    losses = []
    g = torch.Generator(device="cuda").manual_seed(rnd)
    for k in range(20):
        if buf is not None:
            losses.append(trainer.step(*buf.sample(512, step=rnd * 20 + k, layout="nchw_channels_last")))
            continue
        idx = torch.randint(0, n, (min(512, n),), generator=g, device="cuda")
        losses.append(trainer.step(states[idx], policies[idx], values[idx]))
    trainer.end_epoch()
    torch.cuda.synchronize()
    t_tr = time.perf_counter() - t0
    if gate > 0:
        from hive_alphazero_amd.arena import Arena
        candidate = InferenceNet(net.eval(), dtype=evaluator.dtype)
        match = Arena(candidate, evaluator, pairs=gate, sims=sims, seed=1000 + rnd)
        verdict = match.run()
        assert match.illegal_count() == 0
        match.close()
        print(f"round {rnd}: gate {verdict!r} -> {'refresh' if verdict.passes() else 'keep the old weights'}", flush=True)
        if verdict.passes():
            evaluator.refresh(net)
    else:
        evaluator.refresh(net)
    print(f"round {rnd}: {sp.plies} {'turn-overs' if opts.rolling else 'plies'} of {games} games x {sims} sims in {t_sp:.1f} s, W/B/draw {results}, illegal {illegal}; "
          + (f"{n} rows of {records.packed_games(packed)} games widened on the GPU in {t_ds * 1e3:.0f} ms; " if buf is None else
             f"{n} rows of {records.packed_games(packed)} games appended to the replay window in {t_ds * 1e3:.0f} ms "
             f"(fill {len(buf)} / {buf.capacity} rows, {buf.rows_seen} seen); ") +
          (f"{len(packed['meta'])} plies, {n} of them full; " if cap else "") +
          f"20 training steps of 512 in {t_tr:.1f} s, loss {losses[0]:.3f} -> {losses[-1]:.3f}", flush=True)
    assert illegal == 0 and all(np.isfinite(l) for l in losses) and records.packed_games(packed) == games
print("ok")
