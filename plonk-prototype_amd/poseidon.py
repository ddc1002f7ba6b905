"""Native Poseidon on the GPU (``pm_hades_*`` / ``pm_poseidon_*``): the Hades permutation of width 5
outside a circuit, the modelled sponge of rate 4 on top of it and an arity-4 Merkle tree with batched sibling paths, in-place
leaf updates that hash only the changed leaves' ancestors and the bulk verification of paths (section 7.2n), and the append-only
tree of ledger height that stores only what is filled (``LedgerTree``, section 7.2r).

Field elements cross this interface as Montgomery limbs, ``uint64`` arrays with a last axis of 4 (``field.fr_vec_to_limbs``);
constants and the capacity may also be given as Python integers.  With ``Hades.from_key`` the constants are those of a key's own
HADES gadget, so the native hash equals what the gadget's rows constrain."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .field import fr_to_limbs, fr_vec_to_limbs
from .host import Context, DeviceVector, _DeviceView, _p

WIDTH = _lib.PLONK_HADES_WIDTH
FORMS = {"auto": _lib.HADES_FORM_AUTO, "thread": _lib.HADES_FORM_THREAD, "wave": _lib.HADES_FORM_WAVE}


def _elements(x, count: int | None = None) -> np.ndarray:
    """limbs (a uint64 array, last axis 4) or nested integers -> [count, 4] Montgomery limbs"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        a = np.ascontiguousarray(x).reshape(-1, 4)
    else:
        a = fr_vec_to_limbs([int(v) for v in np.asarray(x, dtype=object).reshape(-1)])
    if count is not None and a.shape[0] != count:
        raise ValueError(f"expected {count} field elements, got {a.shape[0]}")
    return a


def _form(form) -> int:
    return FORMS[form] if isinstance(form, str) else int(form)


def _capacity(capacity) -> np.ndarray:
    return fr_to_limbs(capacity) if isinstance(capacity, int) else _elements(capacity, 1).reshape(4)


def hades_permute_host(ark, mds, state, rounds: int = 67, full_rounds: int = 8) -> np.ndarray:
    """``pm_hades_permute_host``: one permutation on the CPU, no context.  ``mds``: one 5 x 5 matrix or ``rounds`` of them."""
    lib = _lib.load()
    a, m = _elements(ark), _elements(mds)
    s = _elements(state, WIDTH).copy()
    if a.shape[0] != WIDTH * rounds or m.shape[0] % 25:
        raise ValueError("the constants do not have the shape of (rounds, full_rounds)")
    if lib.pm_hades_permute_host(rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(s)) != _lib.PM_OK:
        raise ValueError("pm_hades_permute_host refused its arguments")
    return s


def poseidon_hash_host(ark, mds, message, capacity=0, rounds: int = 67, full_rounds: int = 8) -> np.ndarray:
    """``pm_poseidon_hash_host``: the modelled sponge over one message on the CPU -> [4] limbs"""
    lib = _lib.load()
    a, m, msg, cap = _elements(ark), _elements(mds), _elements(message), _capacity(capacity)
    out = np.zeros(4, np.uint64)
    if a.shape[0] != WIDTH * rounds or m.shape[0] % 25:
        raise ValueError("the constants do not have the shape of (rounds, full_rounds)")
    rc = lib.pm_poseidon_hash_host(rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(cap), _p(msg), msg.shape[0], _p(out))
    if rc != _lib.PM_OK:
        raise ValueError("pm_poseidon_hash_host refused its arguments")
    return out


class Hades:
    """The constants of one Hades permutation on a context's GPU (``pm_hades_params``) and what runs with them.

    ``Hades(ctx, ark, mds, rounds=67, full_rounds=8)``: ``ark`` holds ``rounds`` x 5 round keys, ``mds`` one 5 x 5 matrix
    (dusk-hades) or ``rounds`` of them.  ``form`` is ``"auto"``, ``"thread"`` (one permutation per lane) or ``"wave"`` (25 lanes
    per permutation); the bytes do not depend on it."""

    def __init__(self, ctx: Context, ark, mds, rounds: int = 67, full_rounds: int = 8):
        a, m = _elements(ark), _elements(mds)
        if a.shape[0] != WIDTH * rounds or m.shape[0] % 25:
            raise ValueError("ark must hold rounds x 5 elements and mds whole 5 x 5 matrices")
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_hades_params_create(ctx._h, rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, C.byref(h)))
        self._bind(ctx, h)

    def _bind(self, ctx, h):
        self.ctx, self._h = ctx, h
        r, f, k = C.c_uint32(), C.c_uint32(), C.c_uint32()
        ctx._check(ctx._lib.pm_hades_params_info(h, C.byref(r), C.byref(f), C.byref(k)))
        self.rounds, self.full_rounds, self.n_mds = r.value, f.value, k.value

    @classmethod
    def from_key(cls, pk, gadget_index: int) -> "Hades":
        """``pm_hades_params_from_key``: the constants of gadget ``gadget_index`` of ``pk``'s gadget table (kind HADES).  The
        result does not depend on the key afterwards."""
        ctx = pk.ctx
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_hades_params_from_key(ctx._h, pk._h, int(gadget_index), C.byref(h)))
        self = object.__new__(cls)
        self._bind(ctx, h)
        return self

    def free(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_hades_params_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # ------------------------------------------------------------------ device forms (addresses as integers; asynchronous)
    def permute_dev(self, d_states: int, n: int, form="auto", stream: int = 0):
        """``pm_hades_permute_dev``: ``n`` states of 5 elements at ``d_states``, in place"""
        c = self.ctx
        c._check(c._lib.pm_hades_permute_dev(c._h, self._h, C.c_void_p(d_states), n, _form(form), C.c_void_p(stream)))

    def hash_dev(self, d_msgs: int, msg_len: int, n: int, d_out: int, capacity=0, msg_stride: int | None = None, form="auto",
                 stream: int = 0):
        """``pm_poseidon_hash_dev``: ``n`` messages of ``msg_len`` elements, ``msg_stride`` (default ``msg_len``) apart"""
        c = self.ctx
        stride = msg_len if msg_stride is None else msg_stride
        c._check(c._lib.pm_poseidon_hash_dev(c._h, self._h, _p(_capacity(capacity)), C.c_void_p(d_msgs), msg_len, stride, n,
                                             C.c_void_p(d_out), _form(form), C.c_void_p(stream)))

    def merkle_dev(self, d_leaves: int, height: int, d_tree: int, capacity=0, form="auto", stream: int = 0):
        """``pm_poseidon_merkle_dev``: 4^height leaves -> levels 1..height at ``d_tree``, (4^height - 1) / 3 elements"""
        c = self.ctx
        c._check(c._lib.pm_poseidon_merkle_dev(c._h, self._h, _p(_capacity(capacity)), C.c_void_p(d_leaves), height,
                                               C.c_void_p(d_tree), _form(form), C.c_void_p(stream)))

    # ------------------------------------------------------------------ host arrays in, host arrays out
    def permute(self, states, form="auto") -> np.ndarray:
        """[n, 5, 4] limbs -> the permuted states"""
        a = _elements(states)
        if a.shape[0] % WIDTH:
            raise ValueError("states must hold whole states of 5 elements")
        d = DeviceVector.from_host(self.ctx, a)
        try:
            self.permute_dev(d.ptr, a.shape[0] // WIDTH, form)
            return d.to_host().reshape(-1, WIDTH, 4)
        finally:
            d.free()

    def hash(self, messages, capacity=0, form="auto") -> np.ndarray:
        """[n, msg_len, 4] limbs (equal-length messages; [msg_len, 4] is one message) -> [n, 4] hashes"""
        a = np.ascontiguousarray(messages, dtype=np.uint64)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[2] != 4 or a.shape[1] == 0:
            raise ValueError("messages must have the shape [n, msg_len >= 1, 4]")
        n, msg_len = a.shape[0], a.shape[1]
        d, out = DeviceVector.from_host(self.ctx, a), DeviceVector(self.ctx, n)
        try:
            self.hash_dev(d.ptr, msg_len, n, out.ptr, capacity, form=form)
            return out.to_host()
        finally:
            d.free(), out.free()

    def merkle(self, leaves, capacity=0, form="auto") -> "MerkleTree":
        """[4^h, 4] limbs, 1 <= h <= 15 -> the tree over them"""
        a = _elements(leaves)
        height = (a.shape[0].bit_length() - 1) // 2
        if a.shape[0] != 4 ** height or height < 1:
            raise ValueError("the number of leaves must be 4^h with h >= 1")
        d_leaves = DeviceVector.from_host(self.ctx, a)
        d_tree = DeviceVector(self.ctx, (4 ** height - 1) // 3)
        self.merkle_dev(d_leaves.ptr, height, d_tree.ptr, capacity, form)
        return MerkleTree(self.ctx, d_leaves, d_tree, height, hades=self, capacity=capacity)

    def verify_paths_dev(self, d_paths: int, d_indices: int, k: int, height: int, d_root: int, d_status: int, capacity=0,
                         form="auto", stream: int = 0):
        """``pm_poseidon_merkle_verify_dev``: k paths of ``height`` x 4 elements -> k uint32 at ``d_status``; asynchronous"""
        c = self.ctx
        c._check(c._lib.pm_poseidon_merkle_verify_dev(c._h, self._h, _p(_capacity(capacity)), C.c_void_p(d_paths),
                                                      C.c_void_p(d_indices), k, height, C.c_void_p(d_root), C.c_void_p(d_status),
                                                      _form(form), C.c_void_p(stream)))

    def verify_paths(self, paths, indices, root, height: int, capacity=0, form="auto") -> np.ndarray:
        """[k, height, 4, 4] limbs as ``MerkleTree.paths`` gives them, k leaf indices and the root ([4] limbs or an integer)
        -> [k] uint32: 0 = the path folds to the root, 1 = the index is not below 4^height, 2 + l = the hash of level l is
        not the child the next level (the root after the last) holds at the path's position"""
        return _verify_paths(self.ctx, self.verify_paths_dev, paths, indices, root, height, capacity, form)

    # ------------------------------------------------------------------ the append-only tree (section 7.2r)
    def ledger(self, height: int, capacity=0, empty_leaf=0, reserve: int = 0) -> "LedgerTree":
        """``pm_poseidon_ledger_create``: an empty append-only tree of arity 4 and ``height`` (1 .. 31) with room for ``reserve``
        leaves; ``empty_leaf`` is what an unfilled position holds"""
        return LedgerTree(self, height, capacity, empty_leaf, reserve)

    def verify_ledger_paths_dev(self, d_paths: int, d_indices: int, k: int, height: int, d_root: int, d_status: int, capacity=0,
                                form="auto", stream: int = 0):
        """``pm_poseidon_ledger_verify_dev``: ``verify_paths_dev`` for heights up to 31; asynchronous"""
        c = self.ctx
        c._check(c._lib.pm_poseidon_ledger_verify_dev(c._h, self._h, _p(_capacity(capacity)), C.c_void_p(d_paths),
                                                      C.c_void_p(d_indices), k, height, C.c_void_p(d_root), C.c_void_p(d_status),
                                                      _form(form), C.c_void_p(stream)))

    def verify_ledger_paths(self, paths, indices, root, height: int, capacity=0, form="auto") -> np.ndarray:
        """``verify_paths`` for a tree of ledger height (1 .. 31): the same status words"""
        return _verify_paths(self.ctx, self.verify_ledger_paths_dev, paths, indices, root, height, capacity, form)


def _verify_paths(ctx, verify_dev, paths, indices, root, height: int, capacity, form) -> np.ndarray:
    """host arrays through one of the two verification entries (``verify_dev``: a bound ``*_paths_dev`` method) -> [k] uint32"""
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    k = idx.shape[0]
    if k == 0:
        return np.zeros(0, np.uint32)
    a = _elements(paths, k * height * 4)
    d_paths, d_root = DeviceVector.from_host(ctx, a), DeviceVector.from_host(ctx, _capacity(root).reshape(1, 4))
    d_idx, d_status = _upload_words(ctx, idx), DeviceVector(ctx, (k + 7) // 8)
    try:
        verify_dev(d_paths.ptr, d_idx.ptr, k, height, d_root.ptr, d_status.ptr, capacity, form)
        return d_status.to_host().view(np.uint32).reshape(-1)[:k].copy()
    finally:
        d_paths.free(), d_root.free(), d_idx.free(), d_status.free()


def _upload_words(ctx, words: np.ndarray) -> DeviceVector:
    """k uint64 -> device memory, padded to whole elements of 32 bytes"""
    return DeviceVector.from_host(ctx, np.concatenate([words, np.zeros((-words.shape[0]) % 4, np.uint64)]))


class MerkleTree:
    """An arity-4 Poseidon tree in device memory: ``leaves`` (4^height elements) and ``nodes`` (levels 1..height one after the
    other, the root last) as :class:`DeviceVector`; ``level(l)`` is a view of one level.  ``hades`` and ``capacity`` say how it
    was hashed (``Hades.merkle`` passes them): ``update`` and ``verify`` need them."""

    def __init__(self, ctx: Context, leaves: DeviceVector, nodes: DeviceVector, height: int, hades: "Hades | None" = None,
                 capacity=0):
        self.ctx, self.leaves, self.nodes, self.height = ctx, leaves, nodes, height
        self.hades, self.capacity = hades, capacity

    def level(self, l: int) -> DeviceVector:
        if not 0 <= l <= self.height:
            raise ValueError("no such level")
        if l == 0:
            return self.leaves.view(0, self.leaves.n)
        first = sum(4 ** (self.height - q) for q in range(1, l))
        return self.nodes.view(first, 4 ** (self.height - l))

    @property
    def root(self) -> np.ndarray:
        return self.level(self.height).to_host()[0]

    def paths_dev(self, d_indices: int, k: int, d_out: int, stream: int = 0):
        """``pm_poseidon_merkle_paths_dev``: k uint64 indices -> k x height x 4 elements; waits for the stream"""
        c = self.ctx
        c._check(c._lib.pm_poseidon_merkle_paths_dev(c._h, C.c_void_p(self.leaves.ptr), C.c_void_p(self.nodes.ptr), self.height,
                                                     C.c_void_p(d_indices), k, C.c_void_p(d_out), C.c_void_p(stream)))

    def paths(self, indices) -> np.ndarray:
        """-> [k, height, 4, 4]: ``out[j][l][c]`` is child c of the level-(l + 1) ancestor of leaf ``indices[j]``; the path
        node itself is child ``(indices[j] >> 2 l) & 3``"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        k = idx.shape[0]
        if k == 0:
            return np.zeros((0, self.height, 4, 4), np.uint64)
        d_idx = DeviceVector.from_host(self.ctx, np.concatenate([idx, np.zeros((-k) % 4, np.uint64)]))
        out = DeviceVector(self.ctx, k * self.height * 4)
        try:
            self.paths_dev(d_idx.ptr, k, out.ptr)
            return out.to_host().reshape(k, self.height, 4, 4)
        finally:
            d_idx.free(), out.free()

    def _hashed_by(self) -> "Hades":
        if self.hades is None:
            raise ValueError("this tree does not know its Hades constants: build it with Hades.merkle or pass hades=")
        return self.hades

    def update_dev(self, d_indices: int, d_values: int, k: int, d_work: int, form="auto", stream: int = 0) -> int:
        """``pm_poseidon_merkle_update_dev``: k strictly ascending uint64 indices and k elements in device memory, ``d_work``
        of ``pm_poseidon_merkle_update_work_bytes(k)`` bytes -> the permutations run; waits for the stream"""
        h, c = self._hashed_by(), self.ctx
        hashed = C.c_uint64(0)
        c._check(c._lib.pm_poseidon_merkle_update_dev(c._h, h._h, _p(_capacity(self.capacity)), C.c_void_p(self.leaves.ptr),
                                                      C.c_void_p(self.nodes.ptr), self.height, C.c_void_p(d_indices),
                                                      C.c_void_p(d_values), k, C.c_void_p(d_work), _form(form),
                                                      C.byref(hashed), C.c_void_p(stream)))
        return hashed.value

    def update(self, indices, values, form="auto") -> int:
        """leaves[indices[j]] = values[j] ([k, 4] limbs or integers), then only the ancestors of the changed leaves are hashed
        again -> the permutations run.  Any order of indices; a duplicate is a ``ValueError``."""
        self._hashed_by()
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        k = idx.shape[0]
        if k == 0:
            return 0
        vals = _elements(values, k)
        order = np.argsort(idx, kind="stable")
        idx, vals = idx[order], np.ascontiguousarray(vals[order])
        if (idx[1:] == idx[:-1]).any():
            raise ValueError("duplicate leaf indices")
        d_idx, d_vals = _upload_words(self.ctx, idx), DeviceVector.from_host(self.ctx, vals)
        work = DeviceVector(self.ctx, (self.ctx._lib.pm_poseidon_merkle_update_work_bytes(k) + 31) // 32)
        try:
            return self.update_dev(d_idx.ptr, d_vals.ptr, k, work.ptr, form)
        finally:
            d_idx.free(), d_vals.free(), work.free()

    def verify(self, paths, indices, root=None, form="auto") -> np.ndarray:
        """``Hades.verify_paths`` with this tree's constants, capacity and height; ``root`` defaults to the current root"""
        return self._hashed_by().verify_paths(paths, indices, self.root if root is None else root, self.height, self.capacity,
                                              form)

    def free(self):
        self.leaves.free(), self.nodes.free()


class LedgerTree:
    """An append-only Poseidon tree of arity 4 and a fixed ``height`` up to 31 (``pm_poseidon_ledger``):
    leaves are filled from position 0 upward, only nodes with a filled descendant are stored, and everything to the right reads
    as the empty subtree of its level (``empty_roots``).  The device handle keeps its own copy of the constants, so appends,
    truncates, roots and paths go on after the ``Hades`` it came from is freed; ``verify`` runs through that ``Hades`` and needs
    it alive.  Not for concurrent use."""

    def __init__(self, hades: Hades, height: int, capacity=0, empty_leaf=0, reserve: int = 0):
        ctx = hades.ctx
        self.ctx, self.hades, self.capacity, self._h = ctx, hades, capacity, None
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_poseidon_ledger_create(ctx._h, hades._h, _p(_capacity(capacity)), int(height),
                                                      _p(_capacity(empty_leaf)), int(reserve), C.byref(h)))
        self._h, self.height = h, int(height)

    def _info(self):
        count, reserve, nbytes = C.c_uint64(), C.c_uint64(), C.c_size_t()
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_info(self._h, None, C.byref(count), C.byref(reserve), C.byref(nbytes)))
        return count.value, reserve.value, nbytes.value

    @property
    def count(self) -> int:
        return self._info()[0]

    @property
    def reserve(self) -> int:
        return self._info()[1]

    @property
    def device_bytes(self) -> int:
        return self._info()[2]

    @property
    def empty_roots(self) -> np.ndarray:
        """[height + 1, 4] limbs: Z_0 = the empty leaf .. Z_height = the root of the empty tree"""
        out = np.zeros((self.height + 1, 4), np.uint64)
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_empty_roots(self._h, _p(out)))
        return out

    @property
    def root(self) -> np.ndarray:
        """``pm_poseidon_ledger_root``: waits for the context's stream"""
        out = np.zeros(4, np.uint64)
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_root(self.ctx._h, self._h, _p(out), None))
        return out

    def root_dev(self, d_root: int, stream: int = 0):
        """``pm_poseidon_ledger_root_dev``: one element to ``d_root``, ordered on the stream"""
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_root_dev(self.ctx._h, self._h, C.c_void_p(d_root), C.c_void_p(stream)))

    def level(self, l: int) -> DeviceVector:
        """a view of the stored prefix of level ``l`` (0 = the leaves); valid until the tree next grows"""
        p, n = C.c_void_p(), C.c_uint64()
        if not 0 <= l <= self.height:
            raise ValueError("no such level")
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_level(self._h, l, C.byref(p), C.byref(n)))
        v = object.__new__(_DeviceView)
        v.ctx, v.n, v._parent, v._p = self.ctx, n.value, self, C.c_void_p(p.value or 0)
        return v

    def append_dev(self, d_values: int, k: int, form="auto", stream: int = 0) -> int:
        """``pm_poseidon_ledger_append_dev``: k elements in device memory become the next k leaves -> the permutations run;
        asynchronous unless the tree has to grow"""
        hashed = C.c_uint64(0)
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_append_dev(self.ctx._h, self._h, C.c_void_p(d_values), k, _form(form),
                                                                    C.byref(hashed), C.c_void_p(stream)))
        return hashed.value

    def append(self, values, form="auto") -> int:
        """[k, 4] limbs or integers -> the permutations run"""
        vals = _elements(values)
        if vals.shape[0] == 0:
            return 0
        d = DeviceVector.from_host(self.ctx, vals)
        try:
            return self.append_dev(d.ptr, vals.shape[0], form)
        finally:
            d.free()                                                             # waits for the device

    def truncate(self, count: int, form="auto", stream: int = 0) -> int:
        """``pm_poseidon_ledger_truncate_dev``, the rollback: keep the first ``count`` leaves -> the permutations run"""
        hashed = C.c_uint64(0)
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_truncate_dev(self.ctx._h, self._h, int(count), _form(form),
                                                                      C.byref(hashed), C.c_void_p(stream)))
        return hashed.value

    def paths_dev(self, d_indices: int, k: int, d_out: int, stream: int = 0):
        """``pm_poseidon_ledger_paths_dev``: k uint64 indices below the count -> k x height x 4 elements; waits for the stream"""
        self.ctx._check(self.ctx._lib.pm_poseidon_ledger_paths_dev(self.ctx._h, self._h, C.c_void_p(d_indices), k,
                                                                   C.c_void_p(d_out), C.c_void_p(stream)))

    def paths(self, indices) -> np.ndarray:
        """-> [k, height, 4, 4] in the layout of ``MerkleTree.paths``; a sibling that is not stored is its level's empty root"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        k = idx.shape[0]
        if k == 0:
            return np.zeros((0, self.height, 4, 4), np.uint64)
        d_idx, out = _upload_words(self.ctx, idx), DeviceVector(self.ctx, k * self.height * 4)
        try:
            self.paths_dev(d_idx.ptr, k, out.ptr)
            return out.to_host().reshape(k, self.height, 4, 4)
        finally:
            d_idx.free(), out.free()

    def verify(self, paths, indices, root=None, form="auto") -> np.ndarray:
        """``Hades.verify_ledger_paths`` with this tree's constants, capacity and height; ``root`` defaults to the current root"""
        return self.hades.verify_ledger_paths(paths, indices, self.root if root is None else root, self.height, self.capacity, form)

    def free(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_poseidon_ledger_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
