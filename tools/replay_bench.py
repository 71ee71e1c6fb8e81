"""One minibatch of 512 out of a replay window on one MI355X: the fused sampler against indexing dense tensors.

  A  replay.ReplayBuffer.sample(512, ...): draw + gather + widen + scatter in one launch over ~2.9 KB packed rows
     (fp32 and bf16 planes, layout "nchw_channels_last")
  B  what the loop did before: idx = torch.randint(...); states[idx], policies[idx], values[idx] on the dense fp32 tensors
     of records.dataset_tensors_gpu_packed (38.6 KB per row)

Both hold the same synthetic rows.  ONE process, the variants alternate window by window (devices and runs differ by
several per cent); a window is `--batches` minibatches between two events; the median over `--windows` windows is reported.

    python tools/replay_bench.py [--rows 100000] [--batch 512] [--windows 31] [--batches 20] [--markdown]
"""
import argparse, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hive_alphazero_amd import records, replay

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100000, help="rows in the window (dense fp32: 38.6 KB each)")
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--windows", type=int, default=31)
ap.add_argument("--batches", type=int, default=20, help="minibatches per timed window")
ap.add_argument("--markdown", action="store_true")
args = ap.parse_args()
assert args.windows >= 25, "the median of at least 25 windows"


def synthetic_packed(rows, seed=0, game_len=50):
    """A packed batch of `rows` rows without a Python object per row: random feature / history words, policies over 20..80
    distinct columns (an odd stride coprime to 1584 from a random base), games of `game_len` plies."""
    rng = np.random.default_rng(seed)
    clear = ~np.uint64((1 << 31) | (0xFF << 36))
    feat = rng.integers(0, 1 << 56, size=(rows, 144), dtype=np.uint64) & clear
    hist = rng.integers(0, 1 << 32, size=(rows, 4, 2, 6), dtype=np.uint64).astype(np.uint32)
    ply = np.arange(rows) % game_len
    meta = np.stack([np.minimum(ply, 4), ply + 1, ply & 1], axis=1).astype(np.uint8)     # turn odd <-> white (mover 0) moves
    width = rng.integers(20, 81, size=rows)
    ptr = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    row = np.repeat(np.arange(rows), width)
    k = np.arange(ptr[-1]) - ptr[row]
    stride = np.asarray([5, 7, 13, 17, 19, 23, 25, 29])[rng.integers(0, 8, size=rows)]
    idx = ((rng.integers(0, 1584, size=rows)[row] + stride[row] * k) % 1584).astype(np.int16)
    w = (rng.random(ptr[-1]) + 0.1).astype(np.float32)
    val = (w / np.add.reduceat(w, ptr[:-1])[row]).astype(np.float32)
    game_ptr = np.minimum(np.arange(0, rows + game_len, game_len), rows).astype(np.int64)
    game_ptr = game_ptr[:int(np.searchsorted(game_ptr, rows)) + 1]
    games = len(game_ptr) - 1
    return {"feat": feat, "hist": hist, "meta": meta, "pol_idx": idx, "pol_val": val, "pol_ptr": ptr, "game_ptr": game_ptr,
            "game_val": rng.integers(-1, 2, size=games).astype(np.int8), "game_id": np.arange(games, dtype=np.int64)}


packed = synthetic_packed(args.rows)
n, B = args.rows, args.batch
buf = replay.ReplayBuffer(n)
buf.add_packed(packed)
states, policies, values = records.dataset_tensors_gpu_packed(packed, dtype=torch.float32, layout="chw")
check = torch.arange(0, n, max(1, n // 997), device="cuda")
for got, want in zip(buf.gather(check), (states[check], policies[check], values[check])):
    assert torch.equal(got, want), "the window and the dense tensors hold different rows"
gen = torch.Generator(device="cuda").manual_seed(0)
step = [0]


def a_f32():
    step[0] += 1
    return buf.sample(B, step=step[0], dtype=torch.float32, layout="nchw_channels_last")


def a_bf16():
    step[0] += 1
    return buf.sample(B, step=step[0], dtype=torch.bfloat16, layout="nchw_channels_last")


def b_dense():
    idx = torch.randint(0, n, (B,), generator=gen, device="cuda")
    return states[idx], policies[idx], values[idx]


VARIANTS = {"A fused sample, fp32 planes": a_f32, "A fused sample, bf16 planes": a_bf16, "B dense fp32 tensors indexed": b_dense}


def window(fn, batches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(batches):
        out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) / batches * 1e-3


for fn in VARIANTS.values():
    window(fn, args.batches)
times = {k: [] for k in VARIANTS}
for _ in range(args.windows):
    for name, fn in VARIANTS.items():
        times[name].append(window(fn, args.batches))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
written = {"A fused sample, fp32 planes": B * (8064 * 4 + 6336 + 4), "A fused sample, bf16 planes": B * (8064 * 2 + 6336 + 4),
           "B dense fp32 tensors indexed": B * (8064 * 4 + 6336 + 4)}
held = {"A": 144 * 8 + 48 * 4 + 4 + 4 + 4 + 256 * 2 + 256 * 4, "B": 8064 * 4 + 6336 + 4}
base = med["B dense fp32 tensors indexed"]
if args.markdown:
    print(f"| variant (batch {B}, window {n} rows) | us / batch (median of {args.windows}) | min | max | vs B | written TB/s |")
    print("|---|---|---|---|---|---|")
    for k, v in times.items():
        print(f"| {k} | {med[k] * 1e6:.1f} | {min(v) * 1e6:.1f} | {max(v) * 1e6:.1f} | {med[k] / base:.2f} | {written[k] / med[k] / 1e12:.2f} |")
    print(f"\nbytes held per row: A {held['A']}, B {held['B']} ({held['B'] / held['A']:.1f}x)")
print(json.dumps({"rows": n, "batch": B, "windows": args.windows, "batches_per_window": args.batches,
                  "us_per_batch": {k: round(v * 1e6, 2) for k, v in med.items()},
                  "ratio_A_f32_over_B": round(med["A fused sample, fp32 planes"] / base, 3),
                  "ratio_A_bf16_over_B": round(med["A fused sample, bf16 planes"] / base, 3),
                  "written_TBps": {k: round(written[k] / med[k] / 1e12, 3) for k in med},
                  "bytes_held_per_row": held}))
