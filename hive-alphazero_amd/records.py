"""Self-play records in the reference's wire format (first "next" row) and in a compact one.

woker/self_play.py:100-112,178-193 writes `play_<ts>.json` = list of
`[state[12][12][56], policy[1584], value, [game_len, counter]]`; woker/optimize.py:42-65 loads it
and discounts the value by the moves still to come (load_data).  The GPU engine keeps, per ply, the packed 56-bit
features of every game (1,152 B instead of the 64 KB float64 planes), the visit policy and the mover;
this module expands finished games into those entries.

One MI355X plays ~4,000 games/min = ~3,400 rows/s; as JSON that is ~13 GB/min of text (8,064 numbers per row), more than
Python can format.  `save_games / load_games` therefore keep finished games as they leave the GPU -- packed features,
history bitboards, sparse visit policy: ~1.5 KB per row in an .npz -- and `dataset_from_games` / `rows_from_game` expand
them into exactly what the JSON route yields (same planes, same discounted values) when the trainer asks.

There is one record route.  `PlyLog` (plain numpy, no GPU) keeps the engine's per-ply host copies and cuts the games that
end into ONE form, the packed batch (`PACKED_KEYS`); a (value_white, plies, game id) tuple is a view of it (`unpack_game`),
the training value of a row is `packed_values`, and the dataset_* functions are built on those two.  `game_entries` and
`load_data` restate the reference's own two functions and stay independent of all that: the tests compare against them.
"""
import json
import os
from datetime import datetime

import numpy as np

from .config import DISCOUNTED_REWARD


def unpack_features(words, turn, history_planes=None):
    """uint64[144] packed features (+ the raw turn number) -> float64 [12,12,56] planes as
    GamePlay.encode_board returns them.  History planes 36..43 are not part of the packed word; pass
    them (bool [12,12,8]) when the trainer needs them."""
    w = np.asarray(words).astype(np.uint64).reshape(144)
    bits = ((w[:, None] >> np.arange(56, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)
    planes = bits.reshape(12, 12, 56)
    planes[:, :, 31] = float(turn)
    if history_planes is not None:
        planes[:, :, 36:44] = history_planes
    return planes


def history_planes(hist_words, hist_len):
    """uint32[4,2,6] history bitboards of the mover's perspective (+ how many entries are valid) ->
    bool [12,12,8] planes 36..43 (env_hive.py:431-434)."""
    out = np.zeros((12, 12, 8))
    hw = np.asarray(hist_words).astype(np.uint32).reshape(4, 2, 6)
    for age in range(min(int(hist_len), 4)):
        for k in range(2):
            for r in range(6):
                v = int(hw[age, k, r])
                for bit in range(32):
                    if (v >> bit) & 1:
                        out[2 * r + (bit >> 4), bit & 15, 2 * age + k] = 1.0
    return out


def game_entries(plies, value_white):
    """plies: list of (planes [12,12,56], policy [1584], player 'W'/'B') in game order ->
    the reference's data rows (self_play.py:178-191)."""
    counts = {"W": sum(1 for p in plies if p[2] == "W"), "B": sum(1 for p in plies if p[2] == "B")}
    seen = {"W": 0, "B": 0}
    out = []
    for planes, policy, player in plies:
        seen[player] += 1
        value = value_white if player == "W" else -value_white
        if value_white == 0:
            value = -1                      # draw or length cap counts as a loss for both sides
        out.append([np.asarray(planes).tolist(), [float(x) for x in policy], value, [counts[player], seen[player]]])
    return out


def write_game_data_to_file(path, data):    # woker/sl.py:49-60
    with open(path, "wt") as f:
        json.dump(data, f)


def flush_buffer(buffer, datapath="../dataSelf"):       # self_play.py:100-112
    os.makedirs(datapath, exist_ok=True)
    game_id = datetime.now().strftime("%Y%m%d-%H%M%S.%f")
    path = os.path.join(datapath, "play_%s.json" % game_id)
    write_game_data_to_file(path, buffer)
    return path


def load_data(filename):                     # woker/optimize.py:42-65
    with open(filename, "rt") as f:
        data = json.load(f)
    rows = []
    for state, policy, value, game_lens in data:
        game_len, step = game_lens[0], game_lens[1]
        if step != game_len:
            value = value * DISCOUNTED_REWARD ** (game_len - step)
        rows.append([np.array(state), np.array(policy, dtype=np.float32), value])
    return rows


# ------------------------------------------------------------------ compact game files
def rows_from_game(entry):
    """One finished game (value_white, plies[, game id]) as SelfPlay collects it -> the reference's rows."""
    expanded = []
    for words, hist, hlen, turn, policy, mover in entry[1]:
        expanded.append((unpack_features(words, turn, history_planes(hist, hlen)), policy, "W" if mover == 0 else "B"))
    return game_entries(expanded, entry[0])


PACKED_KEYS = ("feat", "hist", "meta", "pol_idx", "pol_val", "pol_ptr", "game_ptr", "game_val", "game_id")
# The one OPTIONAL key of a packed batch: full u8[R], 1 = a training row, 0 = a ply that only moved its game along (the
# fast plies of mcts.SelfPlay(playout_cap=...)).  Such a row stays a row of its game -- the value rule counts the moves of
# a side still to come -- but is no row of a dataset or of the replay window.  A batch without the key is all ones.
FULL_KEY = "full"


def _packed_keys(packed):
    """The keys a container carries for this batch: PACKED_KEYS, and the optional one when the batch has it."""
    return PACKED_KEYS + ((FULL_KEY,) if FULL_KEY in packed else ())


def training_rows(packed):
    """int64[N]: the rows of a packed batch that are training rows, ascending (all of them without the `full` key)."""
    if FULL_KEY not in packed:
        return np.arange(len(packed["meta"]), dtype=np.int64)
    return np.flatnonzero(np.asarray(packed[FULL_KEY]) != 0).astype(np.int64)


def pack_games(games):
    """Finished games (value_white, plies[, game id]) -> the arrays a play_<ts>.npz holds (and the form SelfPlayWorker's
    children send): feat u64[R,144], hist u32[R,4,2,6], meta u8[R,3] = (valid history entries, turn, mover), the visit
    policies as one CSR matrix (pol_ptr i64[R+1], pol_idx i16, pol_val f32), game_ptr i64[G+1] (rows of game g),
    game_val i8[G], game_id i64[G] (-1 = unknown).  Rows are grouped by game, plies ascending."""
    feat, hist, meta, pol, game_ptr, game_val, game_id = [], [], [], [], [0], [], []
    for entry in games:
        for words, hw, hlen, turn, policy, mover in entry[1]:
            feat.append(np.asarray(words, dtype=np.uint64).reshape(144))
            hist.append(np.asarray(hw, dtype=np.uint32).reshape(4, 2, 6))
            meta.append((int(hlen), int(turn), int(mover)))
            pol.append(np.asarray(policy, dtype=np.float32).reshape(1584))
        game_ptr.append(len(feat))
        game_val.append(int(entry[0]))
        game_id.append(int(entry[2]) if len(entry) > 2 else -1)
    pol_ptr, pol_idx, pol_val = _csr(np.stack(pol) if pol else np.zeros((0, 1584), np.float32))
    return {"feat": np.stack(feat) if feat else np.zeros((0, 144), np.uint64),
            "hist": np.stack(hist) if hist else np.zeros((0, 4, 2, 6), np.uint32),
            "meta": np.asarray(meta, dtype=np.uint8).reshape(-1, 3), "pol_idx": pol_idx, "pol_val": pol_val, "pol_ptr": pol_ptr,
            "game_ptr": np.asarray(game_ptr, dtype=np.int64), "game_val": np.asarray(game_val, dtype=np.int8),
            "game_id": np.asarray(game_id, dtype=np.int64)}


def _csr(dense):
    """float32 [R,1584] -> (ptr i64[R+1], column i16[N], value f32[N]) of the non-zero entries, columns ascending per row."""
    r, c = np.nonzero(dense)
    ptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dense.shape[0]), out=ptr[1:])
    return ptr, c.astype(np.int16), dense[r, c].astype(np.float32)


def packed_games(packed):
    return len(packed["game_val"])


def slice_packed(packed, lo, hi):
    """Games lo .. hi-1 of a packed batch as a packed batch of their own."""
    r0, r1 = int(packed["game_ptr"][lo]), int(packed["game_ptr"][hi])
    p0, p1 = int(packed["pol_ptr"][r0]), int(packed["pol_ptr"][r1])
    out = {"feat": packed["feat"][r0:r1], "hist": packed["hist"][r0:r1], "meta": packed["meta"][r0:r1],
           "pol_idx": packed["pol_idx"][p0:p1], "pol_val": packed["pol_val"][p0:p1],
           "pol_ptr": packed["pol_ptr"][r0:r1 + 1] - p0, "game_ptr": packed["game_ptr"][lo:hi + 1] - r0,
           "game_val": packed["game_val"][lo:hi], "game_id": packed["game_id"][lo:hi]}
    if FULL_KEY in packed:
        out[FULL_KEY] = packed[FULL_KEY][r0:r1]
    return out


def concat_packed(batches):
    """Several packed batches -> one (game order = batch order).  If any of them has the `full` key the result has it, and a
    batch without it counts as all ones."""
    batches = list(batches)
    if len(batches) == 1:
        return batches[0]
    if not batches:
        return pack_games([])
    out = {k: np.concatenate([b[k] for b in batches]) for k in ("feat", "hist", "meta", "pol_idx", "pol_val", "game_val", "game_id")}
    for key, unit in (("pol_ptr", "pol_idx"), ("game_ptr", "meta")):
        parts, base = [np.zeros(1, dtype=np.int64)], 0
        for b in batches:
            parts.append(b[key][1:] + base)
            base += len(b[unit])
        out[key] = np.concatenate(parts)
    if any(FULL_KEY in b for b in batches):
        out[FULL_KEY] = np.concatenate([np.asarray(b[FULL_KEY], dtype=np.uint8) if FULL_KEY in b
                                        else np.ones(len(b["meta"]), dtype=np.uint8) for b in batches])
    return out


def unpack_game(packed, g):
    """Game g of a packed batch as SelfPlay collects it: (value_white, plies, game id), plies =
    (features uint64[144], history words uint32[4,2,6], valid entries, turn, dense policy float32[1584], mover)."""
    meta, csr = packed["meta"], (packed["pol_ptr"], packed["pol_idx"], packed["pol_val"])
    plies = [(packed["feat"][r], packed["hist"][r], int(meta[r, 0]), int(meta[r, 1]), _dense_row(csr, r), int(meta[r, 2]))
             for r in range(int(packed["game_ptr"][g]), int(packed["game_ptr"][g + 1]))]
    return (int(packed["game_val"][g]), plies, int(packed["game_id"][g]))


def _dense_row(csr, r):
    """float32[1584]: row r of the (ptr, column, value) form _csr builds."""
    ptr, idx, val = csr
    policy = np.zeros(1584, dtype=np.float32)
    lo, hi = int(ptr[r]), int(ptr[r + 1])
    policy[idx[lo:hi]] = val[lo:hi]
    return policy


class PackedGames:
    """Read-only mapping game id -> (value_white, plies, game id) over packed batches; a game is expanded when it is asked
    for (SelfPlayWorker.results in the compact format: 1024 finished games are 55 k dense 1584-wide policies otherwise)."""

    def __init__(self):
        self._where = {}

    def add(self, packed):
        for g, gid in enumerate(packed["game_id"].tolist()):
            self._where[int(gid)] = (packed, g)

    def add_ids(self, packed):
        """Remember which games were seen and how long they were, not their rows (SelfPlayWorker(keep_results=False))."""
        lens = (packed["game_ptr"][1:] - packed["game_ptr"][:-1]).tolist()
        for g, gid in enumerate(packed["game_id"].tolist()):
            self._where[int(gid)] = (None, lens[g])

    def sort(self):
        self._where = dict(sorted(self._where.items()))

    def __getitem__(self, gid):
        packed, g = self._where[gid]
        if packed is None:
            raise KeyError(f"game {gid} was written to a file and not kept (keep_results=False)")
        return unpack_game(packed, g)

    def __iter__(self):
        return iter(self._where)

    def __len__(self):
        return len(self._where)

    def __contains__(self, gid):
        return gid in self._where

    def keys(self):
        return self._where.keys()

    def values(self):
        return (self[k] for k in self._where)

    def items(self):
        return ((k, self[k]) for k in self._where)

    def rows_of(self, gid):
        """Number of rows (plies) of a game without expanding it."""
        packed, g = self._where[gid]
        if packed is None:
            return int(g)
        return int(packed["game_ptr"][g + 1] - packed["game_ptr"][g])


def save_packed(path, packed, level=1):
    """One packed batch -> one compressed .npz (what np.savez_compressed writes, read back by np.load), ~1.6 KB per row.
    Deflate level 1: 2.5x faster than numpy's fixed level 6 for 9 % larger files -- the writer threads of an 8-GPU
    SelfPlayWorker parent compress ~55 MB/s of records (tests/test_host_cpu.py, parent-ingest soak)."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=level) as z:
        for k in _packed_keys(packed):
            with z.open(k + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(packed[k]), allow_pickle=False)
    return path


def save_games(path, games):
    """Finished games (SelfPlay.finished_games / drain_finished entries) -> one compressed .npz."""
    return save_packed(path, pack_games(games))


def packed_to_blob(packed, path):
    """A packed batch as ONE raw file (arrays back to back, 64-byte aligned) + the layout that finds them again.  The hand-over
    format between a self-play child and the gathering parent (self_play.SelfPlayWorker): 90 MB through a multiprocessing
    queue cost the parent's main thread ~0.5-1.2 s of pipe reads and unpickling per lock-step wave; mapped from a tmpfs
    file it costs a millisecond, and the writer threads compress straight out of the mapping."""
    layout, off = [], 0
    for k in _packed_keys(packed):
        a = np.ascontiguousarray(packed[k])
        layout.append((k, a.dtype.str, tuple(a.shape), off))
        off += (a.nbytes + 63) // 64 * 64
    with open(path, "wb") as f:
        f.truncate(max(off, 1))
        for (k, _, _, o) in layout:
            f.seek(o)
            f.write(np.ascontiguousarray(packed[k]).data)
    return layout


def packed_from_blob(path, layout, unlink=True):
    """Inverse of packed_to_blob: read-only array views into a private mapping of the file.  With `unlink` the name is
    removed at once -- the mapping keeps the bytes alive exactly as long as somebody holds a view."""
    import mmap
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        mm = mmap.mmap(f.fileno(), size, prot=mmap.PROT_READ)
    if unlink:
        os.unlink(path)
    out = {}
    for k, dt, shape, off in layout:
        n = int(np.prod(shape)) if len(shape) else 1
        out[k] = np.frombuffer(mm, dtype=np.dtype(dt), count=n, offset=off).reshape(shape)
    return out


def load_packed(path):
    with np.load(path) as z:                      # plain arrays only: nothing in the file is executed
        return {k: z[k] for k in PACKED_KEYS + ((FULL_KEY,) if FULL_KEY in z.files else ())}


def load_games(path):
    """Inverse of save_games: list of (value_white, plies, game id) with plies as SelfPlay.ply_record builds them."""
    packed = load_packed(path)
    return [unpack_game(packed, g) for g in range(packed_games(packed))]


def packed_values(packed):
    """float32[R]: the training value of every row of a packed batch -- value_white from the mover's side (draw / length cap
    = -1 for both, self_play.py:178-191), discounted by DISCOUNTED_REWARD ** (moves of that side still to come),
    optimize.py:42-65.  THE implementation of that rule for everything built from packed batches (the dataset_* functions
    below; replay.discount_table tabulates it for the device); load_data above is the reference's own statement of it."""
    gp = packed["game_ptr"]
    n = int(gp[-1]) if len(gp) else 0
    gi = np.repeat(np.arange(len(gp) - 1), np.diff(gp))
    mover = packed["meta"][:, 2].astype(np.int64)
    vw = packed["game_val"].astype(np.int64)[gi]
    value = np.where(vw == 0, -1.0, np.where(mover == 0, vw, -vw).astype(np.float64))
    left = np.zeros(n, dtype=np.int64)                        # moves of the row's side after this one
    for side in (0, 1):
        c = np.concatenate([[0], np.cumsum(mover == side)])
        seen = c[1:] - c[gp[:-1]][gi]
        total = (c[gp[1:]] - c[gp[:-1]])[gi]
        left = np.where(mover == side, total - seen, left)
    table = np.asarray([DISCOUNTED_REWARD ** k for k in range(int(left.max()) + 1 if n else 1)])
    return np.where(left > 0, value * table[left], value).astype(np.float32)


def dataset_from_packed(packed):
    """What woker/optimize.py:42-65 builds from the JSON rows, straight from a packed batch: (states float32 [N,12,12,56],
    policies float32 [N,1584], values float32 [N] = packed_values).  With the `full` key: the rows marked 1 only, their
    values still computed over all rows of their games."""
    meta, csr = packed["meta"], (packed["pol_ptr"], packed["pol_idx"], packed["pol_val"])
    rows = training_rows(packed).tolist()
    states = [unpack_features(packed["feat"][r], int(meta[r, 1]), history_planes(packed["hist"][r], int(meta[r, 0]))).astype(np.float32)
              for r in rows]
    if not rows:
        return np.zeros((0, 12, 12, 56), np.float32), np.zeros((0, 1584), np.float32), np.zeros((0,), np.float32)
    return np.stack(states), np.stack([_dense_row(csr, r) for r in rows]), packed_values(packed)[rows]


def dataset_from_games(games):
    """dataset_from_packed for finished games (value_white, plies[, game id]) as SelfPlay / load_games hand them out."""
    return dataset_from_packed(pack_games(games))


def board_records(meta, hist):
    """The rows of a packed batch as the env's records (include/hive_abi.h): boards u8[n,64] with the turn in byte 33 and
    the number of valid history entries in the mover's nibble of byte 35, hist u32[n,2,4,2,6] with the history words in the
    mover's half -- all that hive_expand_launch reads besides the packed features."""
    meta = np.asarray(meta).astype(np.int64)
    n = len(meta)
    hlen, turn, mover = meta[:, 0], meta[:, 1], meta[:, 2]
    boards = np.zeros((n, 64), dtype=np.uint8)
    boards[:, 33] = turn
    boards[:, 35] = np.where(mover == 0, hlen & 15, (hlen << 4) & 255)
    out = np.zeros((n, 2, 4, 2, 6), dtype=np.uint32)
    out[np.arange(n), mover] = hist
    return boards, out


def expand_planes(boards, hist, feat, device, dtype, layout):
    """Host records (board_records' arrays + feat u64[n,144], n >= 1) -> the planes on `device`, widened by the env's own
    plane writer (hive_expand_launch): [n,56,12,12] for layout "chw", else [n,12,12,56]."""
    import torch
    from . import _lib
    n = len(boards)
    planes = torch.empty((n, 56, 12, 12) if layout == "chw" else (n, 12, 12, 56), dtype=dtype, device=device)
    tb = torch.from_numpy(boards).to(device)
    th = torch.from_numpy(hist.view(np.uint8).reshape(n, 384)).to(device)
    tf = torch.from_numpy(np.ascontiguousarray(feat).view(np.int64)).to(device)
    _lib.check(_lib.load().hive_expand_launch(_lib.ptr(tb), _lib.ptr(th), _lib.ptr(tf), n, _lib.ptr(planes), _lib.dtype_code(dtype),
                                              _lib.CHW if layout == "chw" else _lib.HWC, _lib.stream_ptr(device)))
    return planes


def dataset_tensors_gpu_packed(packed, device=None, dtype=None, layout="chw"):
    """dataset_from_packed on the GPU, without a Python object per row (records.load_packed /
    SelfPlay.drain_finished_packed): the packed features, history words and turn bytes go up as they are (1.5 KB per row),
    the env's plane writer widens them, the sparse policies are scattered into the dense matrix on the GPU -- what a trainer
    that keeps up with the self-play GPUs uses.  -> (states [N,56,12,12] ("chw", what ChessNet takes) or [N,12,12,56],
    policies float32 [N,1584], values float32 [N] = packed_values) on `device`.  With the `full` key: the rows marked 1 only,
    their values still computed over all rows of their games."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    dtype = dtype or torch.float32
    values = packed_values(packed)
    if FULL_KEY in packed:
        keep = training_rows(packed)
        ptr = np.asarray(packed["pol_ptr"], dtype=np.int64)
        c = ptr[keep + 1] - ptr[keep]
        new_ptr = np.zeros(len(keep) + 1, dtype=np.int64)
        np.cumsum(c, out=new_ptr[1:])
        src = np.repeat(ptr[keep] - new_ptr[:-1], c) + np.arange(int(new_ptr[-1]))
        packed = {"feat": packed["feat"][keep], "hist": packed["hist"][keep], "meta": packed["meta"][keep],
                  "pol_ptr": new_ptr, "pol_idx": packed["pol_idx"][src], "pol_val": packed["pol_val"][src]}
        values = values[keep]
    n = len(packed["meta"])
    if n == 0:                      # nothing to widen (hive_expand_launch refuses n <= 0)
        shape = (0, 56, 12, 12) if layout == "chw" else (0, 12, 12, 56)
        return (torch.zeros(shape, dtype=dtype, device=dev), torch.zeros((0, 1584), dtype=torch.float32, device=dev),
                torch.zeros((0,), dtype=torch.float32, device=dev))
    planes = expand_planes(*board_records(packed["meta"], packed["hist"]), packed["feat"], dev, dtype, layout)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(packed["pol_ptr"]))
    flat = torch.from_numpy(rows * 1584 + packed["pol_idx"].astype(np.int64)).to(dev)
    policies = torch.zeros((n * 1584,), dtype=torch.float32, device=dev)
    policies[flat] = torch.from_numpy(np.ascontiguousarray(packed["pol_val"])).to(dev)
    return planes, policies.view(n, 1584), torch.from_numpy(np.ascontiguousarray(values)).to(dev)


def dataset_tensors_gpu(games, device=None, dtype=None, layout="chw"):
    """dataset_tensors_gpu_packed for finished games (value_white, plies[, game id])."""
    return dataset_tensors_gpu_packed(pack_games(games), device, dtype, layout)


# ------------------------------------------------------------------ the per-ply host log
class PlyLog:
    """The host side of SelfPlay's records: whole-batch numpy copies of every ply a running game may still need, and the one
    cutter that turns the games ending on a ply into a packed batch (pack_games' arrays, gathered per logged ply with array
    operations: no per-row Python objects).  Plain numpy: the GPU side (copy stream, pinned staging buffers) stays with
    the caller, which hands the staging set in as an opaque `keepalive` and gets it back from `settle`.

    More than `max_finished_kept` games waiting at the caller are dropped and counted (`dropped_games`, one warning); a game
    whose opening was played outside the log (`unlogged[slot]`) is counted in `unrecorded_games` and leaves nothing."""

    IDLE = 1 << 60                   # start ply of a slot that holds no game: nothing of the log belongs to it

    def __init__(self, slots, max_finished_kept=1024):
        self.entries = []                    # one dict per logged ply, oldest first
        self.start_ply = [0] * slots         # ply counter at which the game in each slot started
        self.unlogged = [False] * slots      # opening plies of this slot's game were not logged
        self.max_finished_kept = max_finished_kept
        self.dropped_games = self.unrecorded_games = 0
        self.flagged = False                 # some ply came with `full` flags: the packed batches carry the key

    def append(self, ply, feat, policy, boards, hist, moved, keepalive=None, full=None):
        """One ply of every slot: feat u64[G,144] (or its int64 bits), dense policy f32[G,1584], board records u8[G,64],
        history u32[G,2,4,2,6] (or its 384 bytes per slot), moved bool[G].  The arrays may be views into staging memory that
        `keepalive` owns and that is still being filled: nothing is read before settle / close_games / ply_record.
        full (optional) u8[G]: 1 = this ply of that slot is a training row; the packed batches then carry the `full` key (a ply
        logged without flags counts as all ones).  Entries older than the oldest running game are forgotten."""
        if full is not None:
            self.flagged = True
        self.entries.append({"ply": ply, "full": None if full is None else np.asarray(full), "feat": np.asarray(feat).view(np.uint64), "policy": np.asarray(policy),
                             "boards": np.asarray(boards), "hist": np.asarray(hist).view(np.uint32).reshape(-1, 2, 4, 2, 6),
                             "moved": np.asarray(moved), "keepalive": keepalive})
        oldest = min(self.start_ply)
        while self.entries and self.entries[0]["ply"] < oldest:
            self.entries.pop(0)

    @staticmethod
    def _entry_csr(e):
        """The visit policies of one logged ply (all slots) as CSR, computed once per ply."""
        if "csr" not in e:
            e["csr"] = _csr(e["policy"])
        return e["csr"]

    def settle(self, e):
        """A logged ply whose arrays are complete leaves its staging memory: the sparse policies are kept (the dense
        1584-wide rows, 6.5 MB per ply at 1024 games, are dropped) with copies of the small arrays.  -> the entry's
        keepalive, free for reuse (None if it had none or was settled before)."""
        if "policy" not in e:
            return None
        self._entry_csr(e)
        del e["policy"]
        for k in ("feat", "boards", "hist", "moved") + (("full",) if e.get("full") is not None else ()):
            e[k] = np.array(e[k])
        return e.pop("keepalive", None)

    @classmethod
    def ply_record(cls, entry, g):
        """(packed features uint64[144], history words uint32[4,2,6], valid entries, turn, policy, mover) of slot g at one
        logged ply."""
        turn = int(entry["boards"][g, 33])
        persp = 0 if turn % 2 == 1 else 1
        hl = int(entry["boards"][g, 35])
        hlen = (hl & 15) if persp == 0 else (hl >> 4)
        return (entry["feat"][g].copy(), entry["hist"][g, persp].copy(), hlen, turn, _dense_row(cls._entry_csr(entry), g), persp)

    def idle(self, slot):
        """The slot holds no game from now on."""
        self.start_ply[slot] = self.IDLE

    def close_games(self, slots, winner, ids, ply_now, waiting=0):
        """The games in `slots` have ended (self_play.py:165-191: value_white = +1 / -1 / 0 from winner[slot] = 1 / 2 / other)
        and their slots start over at `ply_now`.  -> their rows as one packed batch (games by ascending position in `slots`,
        rows by ply; a game without a logged row leaves no entry), or None.  `waiting` = games the caller still holds."""
        import warnings
        keep = []                        # (slot, first logged ply, value_white, game id)
        for s in slots:
            start, self.start_ply[s] = self.start_ply[s], ply_now
            unlogged, self.unlogged[s] = self.unlogged[s], False
            if unlogged:
                self.unrecorded_games += 1
                continue
            if waiting + len(keep) >= self.max_finished_kept:
                if self.dropped_games == 0:
                    warnings.warn(f"SelfPlay: more than {self.max_finished_kept} finished games are waiting; call "
                                  "drain_finished() -- further games are dropped (dropped_games counts them)")
                self.dropped_games += 1
                continue
            keep.append((s, start, 1 if winner[s] == 1 else (-1 if winner[s] == 2 else 0), ids[s]))
        return self._pack(keep) if keep else None

    def _pack(self, keep):
        S = np.asarray([k[0] for k in keep], dtype=np.int64)
        start = np.asarray([k[1] for k in keep], dtype=np.int64)
        feat, hist, meta, cnt, pidx, pval, gk, ply, full = [], [], [], [], [], [], [], [], []
        for e in self.entries:
            k = np.flatnonzero(np.asarray(e["moved"])[S] & (e["ply"] >= start))
            if k.size == 0:
                continue
            sl = S[k]
            b = e["boards"]
            turn = b[sl, 33].astype(np.int64)
            persp = np.where(turn % 2 == 1, 0, 1)
            hl = b[sl, 35].astype(np.int64)
            hlen = np.where(persp == 0, hl & 15, hl >> 4)
            feat.append(e["feat"][sl])
            hist.append(e["hist"][sl, persp])
            meta.append(np.stack([hlen, turn, persp], axis=1).astype(np.uint8))
            if self.flagged:
                full.append((e["full"][sl] != 0).astype(np.uint8) if e.get("full") is not None else np.ones(k.size, dtype=np.uint8))
            ptr, idx, val = self._entry_csr(e)
            c = ptr[sl + 1] - ptr[sl]
            src = np.repeat(ptr[sl] - (np.cumsum(c) - c), c) + np.arange(int(c.sum()))
            cnt.append(c)
            pidx.append(idx[src])
            pval.append(val[src])
            gk.append(k)
            ply.append(np.full(k.size, e["ply"], dtype=np.int64))
        if not feat:
            return None
        gk, ply, cnt = np.concatenate(gk), np.concatenate(ply), np.concatenate(cnt)
        order = np.lexsort((ply, gk))                           # rows by game, plies ascending
        old_ptr = np.cumsum(cnt) - cnt
        c = cnt[order]
        new_ptr = np.zeros(len(c) + 1, dtype=np.int64)
        np.cumsum(c, out=new_ptr[1:])
        src = np.repeat(old_ptr[order] - new_ptr[:-1], c) + np.arange(int(new_ptr[-1]))
        rows_per_game = np.bincount(gk, minlength=len(keep))
        has = rows_per_game > 0                                 # a game without a logged row leaves no entry
        game_ptr = np.zeros(int(has.sum()) + 1, dtype=np.int64)
        np.cumsum(rows_per_game[has], out=game_ptr[1:])
        out = {"feat": np.concatenate(feat)[order], "hist": np.concatenate(hist)[order], "meta": np.concatenate(meta)[order],
               "pol_idx": np.concatenate(pidx)[src], "pol_val": np.concatenate(pval)[src], "pol_ptr": new_ptr,
               "game_ptr": game_ptr, "game_val": np.asarray([k[2] for k in keep], dtype=np.int8)[has],
               "game_id": np.asarray([k[3] for k in keep], dtype=np.int64)[has]}
        if self.flagged:
            out[FULL_KEY] = np.concatenate(full)[order]
        return out
