"""TrainingSample / push_trace! (src/memory.jl:20-26,74-87) and the packed sample records that cross
ranks after a self-play phase."""
from dataclasses import dataclass

import numpy as np

BLACK_BIT = 1 << 63


@dataclass
class TrainingSample:
    s: tuple
    π: np.ndarray
    z: float
    t: float
    n: int = 1


def push_trace(mem, trace, gamma):
    """push_trace!(mem, trace, gamma): appends one TrainingSample per position, last position first."""
    n = len(trace)
    wr = 0.0
    for i in reversed(range(n)):
        wr = gamma * wr + trace.rewards[i]
        s = trace.states[i]
        wp = not (s[0] & BLACK_BIT)
        z = wr if wp else -wr
        mem.append(TrainingSample(s, trace.policies[i], z, float(n - i), 1))
    return n


def sample_dtype(num_actions):
    return np.dtype([("key", "<u8", (2,)), ("N", "<i4", (num_actions,)), ("z", "<f8"), ("t", "<f8"), ("game", "<i4"), ("n", "<i4")])


def pack_samples(games, moves, ngames, num_actions, gamma):
    """Engine records -> flat sample array (state key, visit counts, z, t): the on-wire record of the
    trace gather.  z/t follow push_trace! exactly (az_push_trace)."""
    total = sum(games[i].num_moves for i in range(ngames))
    out = np.zeros(total, dtype=sample_dtype(num_actions))
    k = 0
    for i in range(ngames):
        g = games[i]
        wr = 0.0
        for j in reversed(range(g.num_moves)):
            m = moves[g.first_move + j]
            wr = gamma * wr + float(m.reward)
            wp = not (int(m.key[0]) & BLACK_BIT)
            r = out[k + j]
            r["key"] = (m.key[0], m.key[1])
            r["N"] = list(m.N[:num_actions])
            r["z"] = wr if wp else -wr
            r["t"] = float(g.num_moves - j)
            r["game"] = g.game_id
            r["n"] = 1
        k += g.num_moves
    return out


# ---------------------------------------------------------------------------------------------------------
# MemoryBuffer on the device (memory.jl:34-60) and the Trainer's data (learning.jl:98-121)
import ctypes as _C

from . import _lib as _L


class MemoryBuffer:
    """MemoryBuffer(gspec, size): a circular buffer of TrainingSamples in HBM (az_memory_*).

    push_records takes the packed records of a self-play phase (Engine.selfplay_run / gather_records) and does
    push_trace! for every game on the device; get_experience() / last_batch() return device data sets."""

    def __init__(self, gspec, size, device=0):
        self.gspec = gspec
        h = _C.c_void_p()
        _L.check(_L.lib().az_memory_create(gspec.game_id, device, int(size), _C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _L.lib().az_memory_destroy(self._h)
            self._h = None

    __del__ = close

    def push_records(self, games, moves, ngames, nmoves, gamma):
        tb = _L.TraceBuf()
        tb.games, tb.games_cap, tb.num_games = games, ngames, ngames
        tb.moves, tb.moves_cap, tb.num_moves = moves, nmoves, nmoves
        _L.check(_L.lib().az_memory_push(self._h, _C.byref(tb), float(gamma)))

    def push_engine(self, engine, gamma):
        """push_trace! for every game of the engine's last bounded self-play phase, from its device-resident records"""
        _L.check(_L.lib().az_memory_push_engine(self._h, engine._h, float(gamma)))

    def push_samples(self, samples):
        """push!(mem.buf, e) for host TrainingSamples (or raw _lib.Sample records).

        az_sample.pi is indexed by FULL action index.  A host TrainingSample carries either a full-width π (what
        Dataset.samples() returns) or the reference's compact π over the AVAILABLE actions only (what push_trace builds
        from a Trace, memory.jl:74-87): the compact form is scattered through the state's action mask; any other length
        is an error."""
        n = len(samples)
        nA = self.gspec.num_actions()
        arr = (_L.Sample * max(n, 1))()
        for i, e in enumerate(samples):
            if isinstance(e, _L.Sample):
                _C.memmove(_C.byref(arr[i]), _C.byref(e), _C.sizeof(_L.Sample))
                continue
            arr[i].key[0], arr[i].key[1] = int(e.s[0]), int(e.s[1])
            pi = np.asarray(e.π, dtype=np.float64)
            if len(pi) != nA:
                mask = np.asarray(self.gspec.init((int(e.s[0]), int(e.s[1]))).actions_mask(), dtype=bool)
                if len(pi) != int(mask.sum()):
                    raise ValueError("sample %d: π has %d entries, the state has %d available actions of %d" % (i, len(pi), int(mask.sum()), nA))
                full = np.zeros(nA)
                full[mask] = pi
                pi = full
            for a in range(nA):
                arr[i].pi[a] = float(pi[a])
            arr[i].z, arr[i].t, arr[i].n = float(e.z), float(e.t), int(e.n)
        _L.check(_L.lib().az_memory_push_samples(self._h, arr, n))

    def _lens(self):
        a, b = _C.c_int64(), _C.c_int64()
        _L.check(_L.lib().az_memory_length(self._h, _C.byref(a), _C.byref(b)))
        return a.value, b.value

    def __len__(self):
        return self._lens()[0]

    def cur_batch_size(self):
        return self._lens()[1]

    def new_batch(self):
        _L.check(_L.lib().az_memory_new_batch(self._h))

    def empty(self):
        _L.check(_L.lib().az_memory_empty(self._h))

    def dataset(self, last_batch=False, use_symmetries=False, use_position_averaging=False, weighing_policy=_L.WEIGHT_CONSTANT):
        return Dataset(self, last_batch, use_symmetries, use_position_averaging, weighing_policy)

    def get_experience(self):
        """get_experience(mem) as TrainingSample list (host copy; the device path keeps working on Dataset)"""
        with self.dataset() as d:
            return d.samples()

    def last_batch(self):
        with self.dataset(last_batch=True) as d:
            return d.samples()


class Dataset:
    """The (W, X, A, P, V) data of a Trainer plus its samples, resident on the device (az_dataset_*)."""

    def __init__(self, mem, last_batch, use_symmetries, use_position_averaging, weighing_policy):
        self.gspec = mem.gspec
        h = _C.c_void_p()
        _L.check(_L.lib().az_dataset_create(mem._h, 1 if last_batch else 0, 1 if use_symmetries else 0,
                                            1 if use_position_averaging else 0, int(weighing_policy), _C.byref(h)))
        self._h = h
        info = _L.DatasetInfo()
        _L.check(_L.lib().az_dataset_get_info(h, _C.byref(info)))
        self.num_samples, self.sum_n, self.Wtot, self.Wmean, self.Hp = info.num_samples, info.sum_n, info.Wtot, info.Wmean, info.Hp

    def close(self):
        if getattr(self, "_h", None):
            _L.lib().az_dataset_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return self.num_samples

    def raw_samples(self):
        n = self.num_samples
        out = (_L.Sample * max(n, 1))()
        _L.check(_L.lib().az_dataset_read(self._h, 0, n, out, None, None, None, None, None))
        return out

    def samples(self):
        nA = self.gspec.num_actions()
        raw = self.raw_samples()
        return [TrainingSample((int(raw[i].key[0]), int(raw[i].key[1])), np.array(raw[i].pi[:nA]), raw[i].z, raw[i].t, int(raw[i].n))
                for i in range(self.num_samples)]

    def tensors(self):
        """convert_samples: (W, X, A, P, V) Float32 arrays, sample index first (= the reference's last dimension)"""
        n, nA = self.num_samples, self.gspec.num_actions()
        w, h, c = self.gspec.state_dim()
        W = np.zeros(n, dtype=np.float32); X = np.zeros((n, c, h, w), dtype=np.float32)
        A = np.zeros((n, nA), dtype=np.float32); P = np.zeros((n, nA), dtype=np.float32); V = np.zeros(n, dtype=np.float32)
        vp = lambda a: a.ctypes.data_as(_C.c_void_p)
        _L.check(_L.lib().az_dataset_read(self._h, 0, n, None, vp(W), vp(X), vp(A), vp(P), vp(V)))
        return W, X, A, P, V


class TensorDataset(Dataset):
    """The data of a Trainer made from (W, X, A, P, V) tensors the caller converted itself (az_dataset_create_from_tensors):
    W (n,), X (n, C, H, W) as Network.forward_normalized takes it, A and P (n, num_actions), V (n,).  For hosts that step their own
    game -- the 9x9x4 geometry has no replay memory on the device -- or label positions by other means.  Same surface as Dataset,
    but no TrainingSamples stand behind it: samples() and raw_samples() raise."""

    def __init__(self, gspec_or_game_id, W, X, A, P, V, device=0):
        gspec, arrays = self.validate(gspec_or_game_id, W, X, A, P, V)          # before the library is loaded
        self.gspec = gspec
        W, X, A, P, V = arrays
        vp = lambda a: a.ctypes.data_as(_C.c_void_p)
        h = _C.c_void_p()
        _L.check(_L.lib().az_dataset_create_from_tensors(gspec.game_id, int(device), len(W), vp(W), vp(X), vp(A), vp(P), vp(V), _C.byref(h)))
        self._h = h
        info = _L.DatasetInfo()
        _L.check(_L.lib().az_dataset_get_info(h, _C.byref(info)))
        self.num_samples, self.sum_n, self.Wtot, self.Wmean, self.Hp = info.num_samples, info.sum_n, info.Wtot, info.Wmean, info.Hp

    @staticmethod
    def validate(gspec_or_game_id, W, X, A, P, V):
        """(gspec, contiguous float32 arrays) or ValueError: ranks, shapes against the geometry, one sample count, float32-convertible"""
        from .game import GameSpec, spec_of_game_id
        gspec = gspec_or_game_id if isinstance(gspec_or_game_id, GameSpec) else spec_of_game_id(gspec_or_game_id)
        nA = gspec.num_actions()
        w, h, c = gspec.state_dim()
        want = {"W": (), "X": (c, h, w), "A": (nA,), "P": (nA,), "V": ()}
        out = []
        n = None
        for name, a in zip("WXAPV", (W, X, A, P, V)):
            try:
                a = np.asarray(a)
                if a.dtype.kind not in "fiub":
                    raise TypeError("dtype %s" % a.dtype)
                a = np.ascontiguousarray(a, dtype=np.float32)
            except (TypeError, ValueError) as e:
                raise ValueError("%s cannot be converted to float32: %s" % (name, e)) from None
            if a.ndim != 1 + len(want[name]):
                raise ValueError("%s must have %d dimensions (sample index first), got shape %s" % (name, 1 + len(want[name]), a.shape))
            if tuple(a.shape[1:]) != want[name]:
                raise ValueError("%s must have shape (n,%s), got %s" % (name, "".join(" %d," % k for k in want[name]), a.shape))
            if n is None:
                n = a.shape[0]
            elif a.shape[0] != n:
                raise ValueError("%s holds %d samples, W holds %d" % (name, a.shape[0], n))
            out.append(a)
        if n < 1:
            raise ValueError("at least one sample is needed")
        return gspec, out

    def raw_samples(self):
        raise TypeError("a data set made from tensors holds no TrainingSamples: use tensors()")

    def samples(self):
        raise TypeError("a data set made from tensors holds no TrainingSamples: use tensors()")

    @classmethod
    def _adopt(cls, gspec, handle):
        """a TensorDataset around a data-set handle the library built itself (PlaneMemoryBuffer.dataset)"""
        self = cls.__new__(cls)
        self.gspec, self._h = gspec, handle
        info = _L.DatasetInfo()
        _L.check(_L.lib().az_dataset_get_info(handle, _C.byref(info)))
        self.num_samples, self.sum_n, self.Wtot, self.Wmean, self.Hp = info.num_samples, info.sum_n, info.Wtot, info.Wmean, info.Hp
        return self


class PlaneMemoryBuffer:
    """MemoryBuffer(gspec, size) for a game whose rules live on the host (az_plane_memory_*): a circular buffer in HBM of what such a
    game can give -- per sample the planes X (C, H, W) and the mask A (num_actions,) the network sees, π by FULL action index, z, t
    and n.  Any of the four geometries; Go9PlanesSpec is the reason for it.

    Two samples are one state when their (X, A) rows are bit-identical.  dataset() merges them (use_position_averaging), converts
    them (convert_samples, learning.jl:17-51) and returns a TensorDataset, all on the device: Trainer takes it as it is."""

    def __init__(self, gspec, capacity, device=0):
        self.gspec = gspec
        h = _C.c_void_p()
        _L.check(_L.lib().az_plane_memory_create(gspec.game_id, int(device), int(capacity), _C.byref(h)))
        self._h = h
        self._batch = []                    # (game_id or None, len) of every trace pushed since new_batch: batch_games()

    def close(self):
        if getattr(self, "_h", None):
            _L.lib().az_plane_memory_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _arrays(self, X, A, P):
        nA = self.gspec.num_actions()
        w, h, c = self.gspec.state_dim()
        X = np.ascontiguousarray(X, dtype=np.float32)
        A = np.ascontiguousarray(A, dtype=np.float32)
        P = np.ascontiguousarray(P, dtype=np.float64)
        n = X.shape[0] if X.ndim else -1
        if X.shape != (n, c, h, w):
            raise ValueError("X must have shape (n, %d, %d, %d), got %s" % (c, h, w, X.shape))
        for name, a in (("A", A), ("π", P)):
            if a.shape != (n, nA):
                raise ValueError("%s must have shape (%d, %d), got %s" % (name, n, nA, a.shape))
        return n, X, A, P

    @staticmethod
    def _vector(name, a, n, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (n,):
            raise ValueError("%s must have shape (%d,), got %s" % (name, n, a.shape))
        return a

    def push_samples(self, X, A, π, z, t, n=None):
        """push!(mem.buf, e) for samples the host holds (n: how often each was seen, default 1); cur_batch_size does not move"""
        cnt, X, A, P = self._arrays(X, A, π)
        z, t = self._vector("z", z, cnt, np.float64), self._vector("t", t, cnt, np.float64)
        nv = None if n is None else self._vector("n", n, cnt, np.int64)
        vp = lambda a: a.ctypes.data_as(_C.c_void_p) if a is not None else None
        _L.check(_L.lib().az_plane_memory_push_samples(self._h, cnt, vp(X), vp(A), vp(P), vp(z), vp(t), vp(nv)))

    def push_trace(self, X, A, π, rewards, white_playing, gamma, game_id=None):
        """push_trace!(mem, trace, gamma) (memory.jl:74-87) for one game in playing order: the planes, mask and π of every position,
        white's reward after every move and who was to move.  game_id: the game's GLOBAL id, remembered with its length for the
        current batch (batch_games; what Comm.gather_push_planes sends)"""
        cnt, X, A, P = self._arrays(X, A, π)
        r = self._vector("rewards", rewards, cnt, np.float64)
        wp = self._vector("white_playing", np.asarray(white_playing).astype(bool), cnt, np.uint8)
        vp = lambda a: a.ctypes.data_as(_C.c_void_p)
        _L.check(_L.lib().az_plane_memory_push_trace(self._h, cnt, vp(X), vp(A), vp(P), vp(r), vp(wp), float(gamma)))
        if cnt > 0:
            self._batch.append((None if game_id is None else int(game_id), cnt))

    def batch_games(self):
        """(game_ids, game_lens), int32: the traces pushed with a game_id since new_batch / empty, in push order.  ValueError if one
        of the batch's traces came without an id"""
        if any(g is None for g, _ in self._batch):
            raise ValueError("the current batch holds traces pushed without a game_id")
        return (np.array([g for g, _ in self._batch], dtype=np.int32), np.array([n for _, n in self._batch], dtype=np.int32))

    def _lens(self):
        a, b = _C.c_int64(), _C.c_int64()
        _L.check(_L.lib().az_plane_memory_length(self._h, _C.byref(a), _C.byref(b)))
        return a.value, b.value

    def samples(self):
        """get_experience(mem) on the host: (X, A, π, z, t, n) arrays in buffer order, oldest first"""
        cnt, nA = len(self), self.gspec.num_actions()
        w, h, c = self.gspec.state_dim()
        X = np.zeros((cnt, c, h, w), dtype=np.float32); A = np.zeros((cnt, nA), dtype=np.float32); P = np.zeros((cnt, nA))
        z = np.zeros(cnt); t = np.zeros(cnt); n = np.zeros(cnt, dtype=np.int64)
        vp = lambda a: a.ctypes.data_as(_C.c_void_p)
        _L.check(_L.lib().az_plane_memory_read(self._h, 0, cnt, vp(X), vp(A), vp(P), vp(z), vp(t), vp(n)))
        return X, A, P, z, t, n

    def __len__(self):
        return self._lens()[0]

    def cur_batch_size(self):
        return self._lens()[1]

    def new_batch(self):
        _L.check(_L.lib().az_plane_memory_new_batch(self._h))
        self._batch = []

    def empty(self):
        _L.check(_L.lib().az_plane_memory_empty(self._h))
        self._batch = []

    def set_symmetries(self, xperm, aperm):
        """GI.symmetries of the host's game, declared once (they belong to the game, not to the samples): nsym gather permutations
        xperm (nsym, C*H*W) over the words of a sample's planes and aperm (nsym, num_actions) over the actions,
        X'[w] = X[xperm[k][w]], A'[j] = A[aperm[k][j]], π'[j] = π[aperm[k][j]].  plane_symmetries(gspec) has the tables of the shipped
        geometries.  Empty tables (nsym = 0) clear the set; a row that is not a bijection is refused and the old set stays."""
        nA = self.gspec.num_actions()
        w, h, c = self.gspec.state_dim()
        xperm = np.ascontiguousarray(xperm, dtype=np.int32)
        aperm = np.ascontiguousarray(aperm, dtype=np.int32)
        nsym = xperm.shape[0] if xperm.ndim else -1
        if xperm.shape != (nsym, c * h * w):
            raise ValueError("xperm must have shape (nsym, %d), got %s" % (c * h * w, xperm.shape))
        if aperm.shape != (nsym, nA):
            raise ValueError("aperm must have shape (%d, %d), got %s" % (nsym, nA, aperm.shape))
        vp = lambda a: a.ctypes.data_as(_C.c_void_p) if a.size else None
        _L.check(_L.lib().az_plane_memory_set_symmetries(self._h, nsym, vp(xperm), vp(aperm)))

    @property
    def num_symmetries(self):
        k = _C.c_int32()
        _L.check(_L.lib().az_plane_memory_num_symmetries(self._h, _C.byref(k)))
        return k.value

    def dataset(self, last_batch=False, use_symmetries=False, use_position_averaging=False, weighing_policy=_L.WEIGHT_CONSTANT):
        """get_experience / last_batch -> augment_with_symmetries (over the declared symmetries, images never stored) -> merge_by_state
        -> convert_samples on the device; the caller closes the TensorDataset"""
        if use_symmetries and self.num_symmetries == 0:
            raise ValueError("use_symmetries needs the game's symmetries, which live on the host: declare them once with "
                             "set_symmetries (plane_symmetries(gspec) has those of the shipped geometries)")
        h = _C.c_void_p()
        _L.check(_L.lib().az_dataset_create_from_plane_memory_sym(self._h, 1 if last_batch else 0, 1 if use_symmetries else 0,
                                                                  1 if use_position_averaging else 0, int(weighing_policy), _C.byref(h)))
        return TensorDataset._adopt(self.gspec, h)
