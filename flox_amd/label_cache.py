"""Label-code cache: factorize once, reuse compact codes across reductions.

The LDS-binned kernel reads 8 B/row of int64 labels only to use them as an
index below ~4e4. The same ``by`` tensor is typically reduced many times
(every variable of a Dataset; mean, then var, then count; both passes of
var), so from the second sighting on the kernel also writes each row's final
group code as uint16 (2 B/row) and later calls read that stream instead. From
``PACK_MIN_ROWS`` rows on, the emitted codes are repacked once to the width
the group count needs (12 bits up to 4094 groups, 14 bits up to 16382:
1.5 / 1.75 B/row, in whole 1024-row tiles) and the uint16 stream is freed —
the device-side analogue of xarray's GroupBy factorizing once, and of the
reference's memoize cache for label-derived work (flox/cache.py).

Policy by sighting of a key:
  1st  record the key only; the call runs exactly the uncached kernel, so a
       one-shot reduction costs nothing extra                       (miss)
  2nd  the ordinary kernel also emits the codes; they are stored    (emit)
  3rd+ the code kernel (uint16 or packed) runs                      (hit)

Key: the caller's ``by`` tensor OBJECT(S) — held by weak reference and
compared by identity, never by address alone (the allocator hands freed
addresses out again) — plus ``_version``, data_ptr, storage offset, shape,
strides, dtype, device and the group shape. Tensors made under
``torch.inference_mode()`` carry no version counter and are never cached. An in-place write through torch bumps ``_version`` and
drops the entry; the death of a label tensor drops it through the weak
reference callback. Writes that bypass torch (a DLPack consumer, a foreign
kernel) do NOT bump ``_version``: turn the cache off around such code with
``set_options(label_cache=False)`` or call ``clear_label_cache()``.

The cache is bounded (LRU over an entry limit and a byte budget) and is
neither read nor written while a stream is being captured: a captured
graph's label buffer is a static input the user may refill in place, and
codes baked into the graph would go stale.

This module holds policy only (no kernels, no GPU calls), so it runs on CPU
tensors too; ``aggregate_hip.grouped_partials`` builds and consumes the codes.
"""

from __future__ import annotations

import threading
import weakref
from collections import OrderedDict

FIRST, EMIT, HIT = "first", "emit", "hit"

DEFAULT_MAX_ENTRIES = 8
DEFAULT_MAX_BYTES = 8 << 30  # codes are at most 2 B/row: 4e9 rows of labels

CODE_BYTES = 2  # uint16

# packed codes (include/floxhip_codes.h). Below PACK_MIN_ROWS rows the uint16
# form is kept (option label_code_pack_min_rows). Default: measured at 1e7,
# 3e7 and 1e8 rows, packed was 4 % slower at 3e7 and 4 % faster at 1e8, the
# smallest size from which it was never slower (profiles/r06_packed_codes.md)
TILE_ROWS = 1024
PACK_MIN_ROWS = 100_000_000


def code_width(ngroups: int, nrows: int) -> int:
    """Bits per cached code for a call: 12 or 14 where the group count leaves
    the all-ones code of that width free and the call is large enough to
    pack, else 16 (uint16)."""
    if nrows < PACK_MIN_ROWS:
        return 16
    return 12 if ngroups <= 4094 else 14 if ngroups <= 16382 else 16


def code_bytes(nrows: int, width: int) -> int:
    """Bytes of the code stream: whole 1024-row tiles for a packed width
    (what fh_packed_code_bytes returns), 2 B/row for uint16."""
    if width == 16:
        return int(nrows) * CODE_BYTES
    return -(-int(nrows) // TILE_ROWS) * (TILE_ROWS // 8) * width


class _Entry:
    __slots__ = ("key", "refs", "sig", "codes", "event", "stream", "nbytes", "width")

    def __init__(self, key, refs, sig, nbytes, width=16):
        self.key = key
        self.refs = refs
        self.sig = sig
        self.codes = None   # uint16[n], or the packed tiles, once emitted
        self.event = None   # recorded after the emitting call (and its packer)
        self.stream = None  # the emitting stream
        self.nbytes = nbytes
        self.width = width  # bits per code: 16, 14 or 12


class Plan:
    """What one call should do: ``action`` is FIRST (run uncached), EMIT
    (run uncached and hand the codes to ``publish``) or HIT (read
    ``codes``, ``width`` bits each; wait on ``event`` when on another stream
    than ``stream``)."""

    __slots__ = ("action", "entry", "codes", "event", "stream", "width")

    def __init__(self, action, entry=None):
        self.action = action
        self.entry = entry
        # snapshot under the cache lock: a concurrent drop clears the entry
        self.codes = entry.codes if entry is not None else None
        self.event = entry.event if entry is not None else None
        self.stream = entry.stream if entry is not None else None
        self.width = entry.width if entry is not None else 16


def _signature(srcs):
    # the address rides ALONGSIDE identity and version (never alone): a
    # storage swap (``by.data = other``) keeps the object, its version and
    # its shape, but not its data_ptr
    return tuple(
        (t._version, t.data_ptr(), t.storage_offset(), tuple(t.shape),
         tuple(t.stride()), t.dtype, str(t.device))
        for t in srcs
    )


class LabelCodeCache:
    def __init__(self, max_entries=DEFAULT_MAX_ENTRIES, max_bytes=DEFAULT_MAX_BYTES):
        self.enabled = True
        self.max_entries = int(max_entries)
        self.max_bytes = int(max_bytes)
        # the weak-reference callback can fire (GC) while this thread holds
        # the lock: reentrant
        self._lock = threading.RLock()
        self._entries: OrderedDict = OrderedDict()
        self._bytes = 0
        self.hits = self.emits = self.misses = 0

    # -- bookkeeping (call with the lock held) ------------------------------
    def _drop(self, key):
        e = self._entries.pop(key, None)
        if e is not None and e.codes is not None:
            self._bytes -= e.nbytes
            e.codes = e.event = e.stream = None

    def _evict(self, keep=None):
        while self._entries and (
            len(self._entries) > self.max_entries or self._bytes > self.max_bytes
        ):
            # snapshot the keys: a weak-reference callback fired by GC on this
            # thread re-enters through the RLock and may drop entries
            victim = next((k for k in list(self._entries) if k != keep), None)
            if victim is None:
                break
            self._drop(victim)

    def _on_dead(self, key):
        with self._lock:
            e = self._entries.get(key)
            if e is not None and any(r() is None for r in e.refs):
                self._drop(key)

    # -- the policy ---------------------------------------------------------
    def acquire(self, srcs, groups, nrows, nbytes=None, width=16):
        """Look the label tensors ``srcs`` (the caller's ``by`` objects) up.
        ``groups``: ngroups, or (g0, g1) for the fused two-by form.
        ``nbytes``: what the codes of this call would occupy (default: uint16,
        2 B/row) and ``width`` their bits per code; an entry made for another
        width (the packing threshold moved) starts over. Returns a
        Plan, or None when the cache is off or the tensors cannot be cached:
        an inference tensor has no version counter, so writes to it could
        not be seen (reading ``_version`` raises) — such a ``by`` runs
        uncached, exactly as without the cache."""
        if not self.enabled or any(t.is_inference() for t in srcs):
            return None
        key = (tuple(id(t) for t in srcs), groups)
        sig = _signature(srcs)
        nbytes = int(nrows) * CODE_BYTES if nbytes is None else int(nbytes)
        with self._lock:
            e = self._entries.get(key)
            if e is not None and (
                e.sig != sig or e.width != width
                or any(r() is not t for r, t in zip(e.refs, srcs))
            ):
                # written in place since (``_version``), a different tensor
                # that happens to reuse the id, or another code width: start over
                self._drop(key)
                e = None
            if e is None:
                self.misses += 1
                if nbytes > self.max_bytes or self.max_entries < 1:
                    return Plan(FIRST)  # could never be held: do not track
                refs = tuple(
                    weakref.ref(t, lambda _r, k=key: self._on_dead(k)) for t in srcs
                )
                self._entries[key] = _Entry(key, refs, sig, nbytes, width)
                self._evict(keep=key)
                return Plan(FIRST)
            self._entries.move_to_end(key)
            if e.codes is None:
                return Plan(EMIT, e)
            self.hits += 1
            return Plan(HIT, e)

    def publish(self, plan, codes, event=None, stream=None):
        """Store the codes an EMIT call produced."""
        e = plan.entry
        with self._lock:
            if self._entries.get(e.key) is not e or e.codes is not None:
                return  # dropped or filled meanwhile
            e.codes, e.event, e.stream = codes, event, stream
            self._bytes += e.nbytes
            self.emits += 1
            self._evict(keep=e.key)

    def clear(self):
        with self._lock:
            for k in list(self._entries):
                self._drop(k)

    def stats(self):
        with self._lock:
            return {
                "hits": self.hits,
                "emits": self.emits,
                "misses": self.misses,
                "bytes": self._bytes,
                "entries": len(self._entries),
            }

    def configure(self, *, enabled=None, max_entries=None, max_bytes=None):
        with self._lock:
            if enabled is not None:
                self.enabled = bool(enabled)
            if max_entries is not None:
                self.max_entries = int(max_entries)
            if max_bytes is not None:
                self.max_bytes = int(max_bytes)
            self._evict()


CACHE = LabelCodeCache()


def clear_label_cache() -> None:
    """Drop every cached code stream (counters are kept)."""
    CACHE.clear()


def label_cache_stats() -> dict:
    """hits / emits / misses since import, and bytes / entries held now."""
    return CACHE.stats()
