"""Every cache of a weight derivative: one key type, one registry, one lock.

A derivative (packed image, folded / merged layer, view, copied weight) lives on the object it derives from, as
``holder.__dict__[name] = {slot: [entry, ...]}``: `slot` starts with ``str(device)`` (the shallow module copies of
nn.parallel.replicate share the dict, their parameters live on different devices), every entry has a ``.key``.  The key
names the source tensors by ``(data_ptr, _version)``, so an entry goes stale when a source is replaced or written through
its version counter; ``clear`` is for the writes that bypass the counter.  The module that fills a cache ``register``s
its name next to the filling function: ema.ema_update_ refreshes and conv.clear_weight_cache clears over these tables.
"""
import threading
from typing import NamedTuple

#: the one (re-entrant) lock of every cache below: hold it from the lookup to the store
LOCK = threading.RLock()

#: name -> refresher(holder, cache, R) of ema.ema_update_.  Derived caches hold layers: refreshed first, the refresher
#: returns the list of layers it rewrote, whose own caches are visited next.  Pack caches hold images: refreshed last
DERIVED_HOOKS, PACK_HOOKS = {}, {}
#: caches that hold no weight derivative, or one that no captured launch reads and that its next use rebuilds
NOT_WEIGHTS = set()
_PINNED = set()
_PINS = threading.local()


class Key(NamedTuple):
    """`tensors`: (data_ptr, _version) or None per source tensor, in a fixed order; `extra`: whatever else the entry was
    built for (operand split and scales, output count, backend, ...)."""
    tensors: tuple
    extra: tuple = ()


def key_of(*tensors, extra=()):
    # (on the path of every eager launch: tuple.__new__ skips the namedtuple's Python-level constructor)
    return tuple.__new__(Key, (tuple([None if t is None else (t.data_ptr(), t._version) for t in tensors]), extra))


class Entry:
    """A cached tensor (or any bare value) under its key."""
    __slots__ = ("key", "value")

    def __init__(self, key, value):
        self.key, self.value = key, value


def register(name, refresh=None, derived=False, weights=True, pinned=False):
    """Declares the cache `name`.  `weights=False`: NOT_WEIGHTS.  `pinned`: its entries are what pin_packs collects."""
    if not weights:
        NOT_WEIGHTS.add(name)
    else:
        (DERIVED_HOOKS if derived else PACK_HOOKS)[name] = refresh
    if pinned:
        _PINNED.add(name)


class pin_packs:
    """Every packed image looked up or made on this thread inside the block is appended to `keep` (strong references): a
    captured graph bakes the images' addresses in, while the per-layer caches evict beyond their `keep` entries -- the
    capturing loop holds what its graphs point to until it drops them (another thread's recalibrations could
    free them)."""

    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        self.prev = getattr(_PINS, "keep", None)
        _PINS.keep = self.keep
        return self.keep

    def __exit__(self, *exc):
        _PINS.keep = self.prev
        return False


def _pin(entry):
    keep = getattr(_PINS, "keep", None)
    if keep is not None:
        keep.append(entry)
    return entry


def lookup(holder, name, slot, key):
    """The entry of `key`, or None."""
    cache = holder.__dict__.get(name)
    if cache:
        for e in cache.get(slot, ()):
            if e.key == key:
                return _pin(e) if name in _PINNED else e
    return None


def store(holder, name, slot, entry, keep=1):
    """Files `entry`: the slot's entries made from other tensors or versions go, at most `keep` stay (newest last)."""
    cache = holder.__dict__.get(name)
    if cache is None:
        cache = holder.__dict__[name] = {}
    same = [e for e in cache.get(slot, ()) if e.key.tensors == entry.key.tensors]
    cache[slot] = (same + [entry])[-keep:]
    return _pin(entry) if name in _PINNED else entry


def cached(holder, name, slot, key, build, keep=1):
    """lookup, else store(build(key)), under the lock."""
    with LOCK:
        hit = lookup(holder, name, slot, key)
        return hit if hit is not None else store(holder, name, slot, build(key), keep)


def clear(module):
    """Empties every registered cache below `module`; the derived layers go with the caches that held them."""
    names = [*DERIVED_HOOKS, *PACK_HOOKS, *NOT_WEIGHTS]
    with LOCK:
        for m in module.modules():
            for name in names:
                cache = m.__dict__.get(name)
                if cache:
                    cache.clear()
