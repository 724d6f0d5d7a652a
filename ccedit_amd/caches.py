"""The one cache idiom of the host code: small bounded maps from the IDENTITY of tensors to something computed from their bytes."""
from dataclasses import dataclass
from typing import Any, Callable, Union


def tensor_key(tns) -> tuple:
    """Identity + version of a tensor's bytes: address, shape, strides, in-place version counter, dtype."""
    return (tns.data_ptr(), tuple(tns.shape), tuple(tns.stride()), tns._version, tns.dtype)


class PinnedCache:
    """key -> value, where the key is built from `tensor_key` of the tensors the value was computed from and the entry PINS those
    tensors (keeps a reference to them).

    The invariant every user relies on: a key match always means the same bytes.  The key is identity plus version — an in-place
    write bumps `_version`, another shape / stride / dtype is another key — and while the entry lives its sources cannot be freed,
    so the caching allocator can never hand their address to a later tensor (the next clip's hint).  Nothing ever has to be
    invalidated for correctness; `clear()` only releases memory early.

    At most `capacity` entries (an int, or a zero-argument callable that is read at every insertion: a limit that follows a
    setting of the owner).  A NEW key that finds the cache full makes room first: evict="all" drops every entry, evict="oldest"
    drops entries in insertion order until there is room.  A lookup never evicts."""

    def __init__(self, capacity: Union[int, Callable[[], int]], evict: str = "all"):
        if evict not in ("all", "oldest"):
            raise ValueError(f"evict={evict!r}: 'all' or 'oldest'")
        self._capacity = capacity if callable(capacity) else (lambda: capacity)
        self._evict = evict
        self._entries = {}                  # key -> (pins, value), in insertion order

    def get(self, key):
        """The value stored under `key`, or None."""
        ent = self._entries.get(key)
        return None if ent is None else ent[1]

    def put(self, key, pins, value) -> None:
        """Store `value` under `key`; `pins`: the tensor(s) whose storage the key describes, held until the entry is evicted."""
        if key not in self._entries:
            room = max(int(self._capacity()), 1) - 1
            if self._evict == "all" and len(self._entries) > room:
                self._entries.clear()
            while len(self._entries) > room:
                del self._entries[next(iter(self._entries))]
        self._entries[key] = (pins, value)

    def clear(self) -> None:
        self._entries.clear()

    def snapshot(self) -> dict:
        """The entries as they are now (a shallow copy: the pins stay held by it), for `restore`."""
        return dict(self._entries)

    def restore(self, snap: dict) -> None:
        """Put back the entries of `snapshot`, in their order; whatever was stored since is dropped."""
        self._entries = dict(snap)

    def values(self):
        """The stored values, oldest first (the pins are nobody's business)."""
        return (value for _, value in self._entries.values())

    def __len__(self) -> int:
        return len(self._entries)

    def __contains__(self, key) -> bool:
        return key in self._entries

    def __iter__(self):
        return iter(self._entries)


@dataclass
class GraphEntry:
    """What the network wrapper's graph cache stores per conditioning key: made at the key's first (eager) evaluation, filled in
    when the second one is captured, replayed from then on."""
    pins: list                  # the conditioning tensors; after the capture also the cached tensors the graph reads
    x: Any = None               # x, t: the static inputs a replay copies the latent / timestep into
    t: Any = None
    out: Any = None             # the static output, cloned after every replay
    graph: Any = None           # torch.cuda.CUDAGraph

    @property
    def captured(self) -> bool:
        return self.graph is not None
