"""The replay window on the GPU: the most recent self-play rows, kept packed, and minibatches drawn from them in one launch.

AlphaZero trains on a sliding window of the most recent games (woker/optimize.py loads the recent play_*.json files).
`ReplayBuffer` keeps that window in HBM as the engine emits it -- packed features, the mover's history words, the sparse
visit policy: about 2.9 KB per row instead of 38.6 KB of dense fp32 -- in a ring that overwrites its oldest rows, and
`sample` / `gather` turn rows of it into the trainer's tensors with one kernel (csrc/hive_replay.hip): draw, gather, widen
to planes exactly as records.dataset_tensors_gpu_packed does, scatter the policy, write the value.  Nothing on that path
touches the host.

    buf = ReplayBuffer(1_000_000)
    buf.add_packed(selfplay.drain_finished_packed())          # or buf.add_file("play_<ts>.npz")
    states, policies, values = buf.sample(512, step=k, layout="nchw_channels_last")

`RingModel` and `draw_indices` mirror the ring's bookkeeping and the device's index draw in plain Python / numpy; they need
no GPU.
"""
import ctypes

import numpy as np

from . import _lib, records
from .config import DISCOUNTED_REWARD
from .search_rules import _M64, _splitmix, rng_word  # noqa: F401  (replay._splitmix stays a name of this module)

POLICY_CAP = _lib.HIVE_LIST_CAP          # the most edges a position has = the most entries a stored policy row holds
MAX_BLOCKS = 2048                        # workgroups of one sample launch; more rows than this take the stride loop
LAYOUTS = ("chw", "hwc", "nchw_channels_last")


def discount_table():
    """float32[256]: the discount of records.packed_values (the one statement of the training-value rule) tabulated for the
    device: DISCOUNTED_REWARD ** k computed in float64 and rounded once -- a value is +-1 times an entry of it, so the
    device's values are packed_values' bit for bit."""
    return np.asarray([DISCOUNTED_REWARD ** k for k in range(256)], dtype=np.float64).astype(np.float32)


# ------------------------------------------------------------------ mirrors (no GPU)
class RingModel:
    """The ring's bookkeeping as hive_replay_append keeps it: `head` is the slot the next row goes to, `live` the rows in
    the window; logical index 0 is the oldest live row."""

    def __init__(self, capacity):
        if capacity < 1:
            raise ValueError("capacity must be at least 1 row")
        self.capacity, self.head, self.live, self.appended = int(capacity), 0, 0, 0

    def append(self, rows):
        """Append a batch of `rows` rows -> [(row of the batch, slot)] for the rows that are written (the last `capacity`)."""
        rows = int(rows)
        if rows < 0:
            raise ValueError("negative row count")
        skip = max(0, rows - self.capacity)
        written = [(i, (self.head + i) % self.capacity) for i in range(skip, rows)]
        self.head = (self.head + rows) % self.capacity
        self.live = min(self.live + rows, self.capacity)
        self.appended += rows
        return written

    def clear(self):
        self.head = self.live = 0

    @property
    def oldest(self):
        return (self.head - self.live) % self.capacity

    def slot_of(self, logical):
        if not 0 <= logical < self.live:
            raise IndexError(f"logical row {logical} outside the window of {self.live}")
        return (self.oldest + logical) % self.capacity


def draw_indices(seed, step, stream_id, n, live):
    """int64[n]: the logical rows hive_replay_sample draws without an index array.  Entry i is a pure function of
    (seed, step, stream_id, i, live): x = the first output of csrc/hive_rng.hpp's generator keyed by (seed, step,
    stream_id, i); the row is the high half of (x >> 32) * live -- uniform over [0, live) up to 2^-32."""
    if live < 1 or live >= 1 << 32:
        raise ValueError("live must be 1 .. 2^32 - 1")
    x = rng_word(int(seed), int(step), int(stream_id), np.arange(int(n), dtype=np.uint64))
    return (((x >> np.uint64(32)) * np.uint64(live)) >> np.uint64(32)).astype(np.int64)


def check_packed(packed):
    """Refuse a packed batch the ring cannot hold, before anything is uploaded -> (rows, games)."""
    rows, games = len(packed["meta"]), len(packed["game_val"])
    pol_ptr, game_ptr = np.asarray(packed["pol_ptr"]), np.asarray(packed["game_ptr"])
    if len(pol_ptr) != rows + 1 or len(game_ptr) != games + 1 or len(packed["feat"]) != rows or len(packed["hist"]) != rows:
        raise ValueError("packed batch: array lengths do not agree")
    if records.FULL_KEY in packed and len(packed[records.FULL_KEY]) != rows:
        raise ValueError("packed batch: the `full` flags do not cover the rows")
    if rows and (int(game_ptr[-1]) != rows or int(game_ptr[0]) != 0 or np.any(np.diff(game_ptr) < 0)):
        raise ValueError("packed batch: game_ptr does not partition the rows")
    width = np.diff(pol_ptr)
    if rows and (int(width.min()) < 0 or int(pol_ptr[0]) != 0 or int(pol_ptr[-1]) != len(packed["pol_idx"])
                 or len(packed["pol_idx"]) != len(packed["pol_val"])):
        raise ValueError("packed batch: pol_ptr does not partition the policy entries")
    if rows and int(width.max()) > POLICY_CAP:
        raise ValueError(f"packed batch: row {int(width.argmax())} has {int(width.max())} policy entries; a position has at "
                         f"most {POLICY_CAP} edges")
    return rows, games


# ------------------------------------------------------------------ the buffer
class ReplayBuffer:
    """A window of the last `capacity_rows` self-play rows on one GPU.  The device block (about 2.9 KB per row) is
    allocated when the first call needs it; every launch goes to the current stream of `device`."""

    def __init__(self, capacity_rows, device=None):
        self.capacity = int(capacity_rows)
        if not 1 <= self.capacity < 1 << 31:
            raise ValueError("capacity_rows must be 1 .. 2^31 - 1")
        self._device_arg, self._device, self._h = device, None, None
        self.rows_seen = 0
        self.games_seen = 0

    # ---- plumbing
    @property
    def device(self):
        if self._device is None:
            import torch
            d = self._device_arg
            if d is None:
                d = torch.cuda.current_device()
            d = torch.device(d) if not isinstance(d, int) else torch.device("cuda", d)
            self._device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        return self._device

    def _handle(self):
        if self._h is None:
            L = _lib.load()
            h = ctypes.c_void_p()
            table = discount_table()
            _lib.check(L.hive_replay_create(self.device.index, self.capacity, ctypes.c_void_p(table.ctypes.data), ctypes.byref(h)))
            self._h = h
        return self._h

    def _stream(self):
        return _lib.stream_ptr(self.device)

    def _up(self, a, view=None):
        import torch
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(view) if view is not None else a).to(self.device)

    def __len__(self):
        if self._h is None:
            return 0
        live = ctypes.c_int64()
        _lib.check(_lib.load().hive_replay_stats(self._h, ctypes.byref(live), None, None))
        return int(live.value)

    def close(self):
        if self._h is not None:
            _lib.load().hive_replay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        if self._h is not None:
            _lib.check(_lib.load().hive_replay_clear(self._h, self._stream()))

    # ---- rows in
    def add_packed(self, packed):
        """Append one packed batch (SelfPlay.drain_finished_packed, records.load_packed, SelfPlayWorker files): about
        1.5 KB per row go up, one launch files them.  A batch longer than the window keeps its last `capacity` rows; every
        row's value is computed from its whole game.  -> rows in the batch.
        With the optional `full` key (records.FULL_KEY) only the rows marked 1 enter the window, in order; the counters and
        the return value count those rows, and each one's value still comes from all rows of its game."""
        import torch
        rows, games = check_packed(packed)
        rank = None
        if records.FULL_KEY in packed:
            flags = np.asarray(packed[records.FULL_KEY]) != 0
            kept = int(flags.sum())
            rank = np.where(flags, np.cumsum(flags) - 1, -1).astype(np.int64)      # place among the kept rows, -1 = left out
        else:
            kept = rows
        if kept == 0:
            self.games_seen += games
            return 0
        L, h = _lib.load(), self._handle()
        pol_ptr = np.ascontiguousarray(packed["pol_ptr"], dtype=np.int64)
        with torch.cuda.device(self.device):
            t = [self._up(packed["feat"], np.int64), self._up(packed["hist"], np.int32), self._up(packed["meta"]),
                 self._up(packed["pol_idx"]), self._up(packed["pol_val"]), self._up(pol_ptr),
                 self._up(np.asarray(packed["game_ptr"], dtype=np.int64)), self._up(packed["game_val"])]
            if t[2].dtype != torch.uint8 or t[3].dtype != torch.int16 or t[4].dtype != torch.float32 or t[7].dtype != torch.int8:
                raise ValueError("packed batch: meta u8, pol_idx i16, pol_val f32, game_val i8 expected")
            if rank is None:
                _lib.check(L.hive_replay_append(h, *[_lib.ptr(x) for x in t], ctypes.c_void_p(pol_ptr.ctypes.data), rows, games,
                                                self._stream()))
            else:
                _lib.check(L.hive_replay_append_ranked(h, *[_lib.ptr(x) for x in t], ctypes.c_void_p(pol_ptr.ctypes.data),
                                                       _lib.ptr(self._up(rank)), rows, games, kept, self._stream()))
        self.rows_seen += kept
        self.games_seen += games
        return kept

    def add_file(self, path):
        return self.add_packed(records.load_packed(path))

    # ---- minibatches out
    def _launch(self, idx, n, seed, step, stream_id, dtype, layout, want_indices, out=None):
        import torch
        dtype = dtype or torch.float32
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {LAYOUTS}")
        dt = _lib.dtype_code(dtype)
        dev = self.device
        shape = (n, 56, 12, 12) if layout == "chw" else (n, 12, 12, 56)
        if out is None:
            planes = torch.empty(shape, dtype=dtype, device=dev)
            policies = torch.empty((n, _lib.HIVE_ACTIONS), dtype=torch.float32, device=dev)
            values = torch.empty((n,), dtype=torch.float32, device=dev)
        else:                                          # the caller's buffers; whatever they hold is overwritten
            planes, policies, values = out
            if layout == "nchw_channels_last":
                planes = planes.permute(0, 2, 3, 1)
            for t, sh, ty in ((planes, shape, dtype), (policies, (n, _lib.HIVE_ACTIONS), torch.float32), (values, (n,), torch.float32)):
                if tuple(t.shape) != sh or t.dtype != ty or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out: a contiguous {ty} tensor of shape {sh} on {dev} expected")
        drawn = torch.empty((n,), dtype=torch.int64, device=dev) if want_indices else None
        if n:
            if len(self) == 0:
                raise RuntimeError("the replay window is empty")
            p = _lib.ptr
            with torch.cuda.device(dev):
                _lib.check(_lib.load().hive_replay_sample(self._handle(), p(idx), int(seed) & _M64, int(step) & _M64,
                                                          int(stream_id) & _M64, n, dt, _lib.CHW if layout == "chw" else _lib.HWC,
                                                          p(planes), p(policies), p(values), p(drawn), self._stream()))
        if layout == "nchw_channels_last":
            planes = planes.permute(0, 3, 1, 2)        # the HWC memory as NCHW: contiguous in torch.channels_last
        return planes, policies, values, drawn

    def gather(self, idx, dtype=None, layout="chw", out=None):
        """Rows `idx` of the window (0 = the oldest live row; duplicates are fine) -> (states, policies f32[n,1584],
        values f32[n]).  `idx` on the host is range-checked; a device tensor is used as it is (the kernel clamps it).
        `out` = (states, policies, values) to write into instead of new tensors."""
        import torch
        live = len(self)
        if not isinstance(idx, torch.Tensor) or idx.device.type != "cuda":
            host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
            if len(host) and (host.min() < 0 or host.max() >= live):
                raise IndexError(f"row index outside the window of {live} rows")
            idx = torch.from_numpy(host).to(self.device)
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        return self._launch(idx, int(idx.numel()), 0, 0, 0, dtype, layout, False, out)[:3]

    def sample(self, batch, step, seed=0, stream_id=0, dtype=None, layout="chw", return_indices=False, out=None):
        """A minibatch of `batch` rows drawn uniformly (with replacement) on the device: a pure function of (seed, step,
        stream_id) and the window -- `stream_id` lets the ranks of a DDP job draw different rows from one seed.
        -> (states, policies, values[, the drawn logical rows i64[batch]])."""
        if len(self) == 0:
            raise RuntimeError("the replay window is empty")
        res = self._launch(None, int(batch), seed, step, stream_id, dtype, layout, return_indices, out)
        return res if return_indices else res[:3]

    # ---- checkpoints
    def state_dict(self):
        """The live rows, oldest first, as host numpy arrays (np.savez takes the dict as it is): feat u64[n,144],
        hist u32[n,4,2,6], meta u8[n,3], pol_cnt i32[n], pol_idx i16[n,256], pol_val f32[n,256], values f32[n], and the
        counters."""
        import torch
        n = len(self)
        dev = self.device if n else "cpu"
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        feat, hist, meta = z((n, 144), torch.int64), z((n, 48), torch.int32), z((n, 4), torch.uint8)
        cnt, pidx, pval, val = z((n,), torch.int32), z((n, POLICY_CAP), torch.int16), z((n, POLICY_CAP), torch.float32), z((n,), torch.float32)
        if n:
            p = _lib.ptr
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().hive_replay_export(self._h, p(feat), p(hist), p(meta), p(cnt), p(pidx), p(pval), p(val),
                                                          self._stream()))
        return {"feat": feat.cpu().numpy().view(np.uint64), "hist": hist.cpu().numpy().view(np.uint32).reshape(n, 4, 2, 6),
                "meta": np.ascontiguousarray(meta.cpu().numpy()[:, :3]), "pol_cnt": cnt.cpu().numpy(), "pol_idx": pidx.cpu().numpy(),
                "pol_val": pval.cpu().numpy(), "values": val.cpu().numpy(),
                "rows_seen": np.int64(self.rows_seen), "games_seen": np.int64(self.games_seen)}

    def load_state_dict(self, state):
        """Replace the window by a state_dict()'s rows (a window larger than this buffer keeps its newest rows)."""
        import torch
        n = len(state["values"])
        cnt = np.asarray(state["pol_cnt"], dtype=np.int32)
        if n and (cnt.min() < 0 or cnt.max() > POLICY_CAP):
            raise ValueError("state: pol_cnt outside 0 .. %d" % POLICY_CAP)
        self.clear()
        if n:
            meta = np.zeros((n, 4), dtype=np.uint8)
            meta[:, :3] = state["meta"]
            with torch.cuda.device(self.device):
                t = [self._up(np.asarray(state["feat"], dtype=np.uint64).reshape(n, 144), np.int64),
                     self._up(np.asarray(state["hist"], dtype=np.uint32).reshape(n, 48), np.int32), self._up(meta), self._up(cnt),
                     self._up(np.asarray(state["pol_idx"], dtype=np.int16).reshape(n, POLICY_CAP)),
                     self._up(np.asarray(state["pol_val"], dtype=np.float32).reshape(n, POLICY_CAP)),
                     self._up(np.asarray(state["values"], dtype=np.float32))]
                _lib.check(_lib.load().hive_replay_import(self._handle(), *[_lib.ptr(x) for x in t], n, self._stream()))
        self.rows_seen = int(state["rows_seen"])
        self.games_seen = int(state["games_seen"])
