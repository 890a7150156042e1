"""The one cache for tensors derived from weights (packs, folds, W^T, merged q | k | v, fp32 copies ...).

A hit means: these exact live tensors at this version.  `data_ptr()` and `_version` alone do not say that -- a freed tensor's address
can come back with version 0 under the caching allocator -- so an entry either holds its sources alive (`derived`) or lives on the
tensor that owns the storage and dies with it (`derived_on_owner`).  Per-clip activation caches and the in-place bf16 shadows are a
different mechanism and do not come through here."""
import torch


def _sig(t):
    return None if t is None else (t.data_ptr(), t._version, t.storage_offset(), t.shape, t.stride(), t.dtype)


def derived(holder, slot: str, sources, build, extra=(), tag=None):
    """`build()` of `sources` (tensors or None), kept in `holder.__dict__[slot]` as `(key, value, sources)` while every source is the
    same storage, layout and version and `extra` (hashable non-tensor inputs) is equal.  The entry holds the sources, so an equal
    pointer is the same live storage.  `tag`: the slot is a dict of such entries (one per block index, parameter name ...)."""
    key = (*[_sig(t) for t in sources], extra)
    entries = holder.__dict__ if tag is None else holder.__dict__.setdefault(slot, {})
    name = slot if tag is None else tag
    hit = entries.get(name)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = (key, build(), tuple(sources))
        entries[name] = hit
    return hit[1]


def derived_on_owner(t: torch.Tensor, slot: str, tag, build):
    """`build()` of `t`, kept in a dict that lives on the tensor owning t's storage (`t._base` of a view: fresh views of one weight
    share the entry), dies with it and is reset when its version moves (or `owner.data = ...` gave it another storage, which leaves
    the version alone); keyed by `tag` and t's offset / shape / strides / dtype.  It does not hold `t` (a view of the owner stored on
    the owner is a reference cycle).  An owner that takes no attributes: built per call."""
    owner = t._base if t._base is not None else t
    stamp = (owner._version, owner.data_ptr())
    cache = getattr(owner, slot, None)
    if cache is None or cache[0] != stamp:
        cache = (stamp, {})
        try:
            setattr(owner, slot, cache)
        except Exception:
            pass
    key = (tag, t.storage_offset(), t.shape, t.stride(), t.dtype, t._version)
    hit = cache[1].get(key)
    if hit is None:
        with torch.no_grad():
            hit = cache[1][key] = build()
    return hit


def drop(holder, *slots: str) -> None:
    for slot in slots:
        holder.__dict__.pop(slot, None)
