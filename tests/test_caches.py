"""CPU tests of ccedit_amd.caches: the key (identity + version), the pin, the two eviction kinds, the mapping protocol."""
import gc
import weakref

import pytest
import torch

from ccedit_amd.caches import GraphEntry, PinnedCache, tensor_key


def test_key_changes_with_an_in_place_write_and_with_a_reallocation():
    a = torch.zeros(4, 6)
    k0 = tensor_key(a)
    assert tensor_key(a) == k0 and k0[0] == a.data_ptr() and k0[1:3] == ((4, 6), (6, 1))
    a.add_(1.0)
    k1 = tensor_key(a)
    assert k1 != k0 and k1[:3] == k0[:3], "an in-place write must change the key through the version alone"
    assert tensor_key(a.t()) != k1, "the same storage with other strides is another key"
    assert tensor_key(a.view(torch.int32)) != k1, "the same storage read as another dtype is another key"
    a = torch.zeros(3, 8)                   # a re-allocation at a different shape (wherever the allocator puts it)
    assert tensor_key(a) != k1 and tensor_key(a)[1] == (3, 8)


def test_an_entry_keeps_its_source_alive_until_it_is_evicted():
    cache = PinnedCache(2)
    src = torch.ones(16)
    alive = weakref.ref(src)
    cache.put(tensor_key(src), src, "computed from src")
    key = tensor_key(src)
    del src
    gc.collect()
    assert alive() is not None and cache.get(key) == "computed from src", "the entry must pin its source"
    other = torch.ones(16)
    assert tensor_key(other)[0] != key[0], "a pinned source's address was handed out again"
    cache.put(tensor_key(other), other, "b")          # room for two: nothing evicted
    assert alive() is not None
    third = torch.ones(16)
    cache.put(tensor_key(third), third, "c")          # full: evict="all" drops both
    gc.collect()
    assert alive() is None and cache.get(key) is None


def test_evict_all_clears_on_a_new_key_at_capacity_and_never_on_a_hit():
    cache = PinnedCache(3)
    for i in range(3):
        cache.put(("k", i), None, i)
    assert len(cache) == 3 and [cache.get(("k", i)) for i in range(3)] == [0, 1, 2], "a hit at capacity must not clear"
    cache.put(("k", 1), None, 10)                       # an existing key at capacity: replaced in place
    assert len(cache) == 3 and cache.get(("k", 1)) == 10
    assert cache.get(("k", 3)) is None and len(cache) == 3, "a miss must not clear either"
    cache.put(("k", 3), None, 3)
    assert list(cache) == [("k", 3)] and list(cache.values()) == [3]


def test_evict_oldest_drops_entries_in_insertion_order():
    cache = PinnedCache(2, evict="oldest")
    cache.put("a", None, 1)
    cache.put("b", None, 2)
    assert cache.get("a") == 1                          # a lookup does not refresh an entry's age
    cache.put("c", None, 3)
    assert list(cache) == ["b", "c"]
    cache.put("b", None, 20)                            # an existing key keeps its place
    cache.put("d", None, 4)
    assert list(cache) == ["c", "d"] and "b" not in cache
    with pytest.raises(ValueError):
        PinnedCache(2, evict="newest")


def test_a_callable_capacity_is_read_again_at_every_insertion():
    limit = [2]
    cache = PinnedCache(lambda: limit[0], evict="oldest")
    for i in range(2):
        cache.put(i, None, i)
    limit[0] = 4                                        # grown: two more fit
    for i in range(2, 4):
        cache.put(i, None, i)
    assert list(cache) == [0, 1, 2, 3]
    limit[0] = 2                                        # shrunk: the next new key makes room down to the new limit
    cache.put(4, None, 4)
    assert list(cache) == [3, 4]
    flush = PinnedCache(lambda: limit[0])
    limit[0] = 3
    for i in range(3):
        flush.put(i, None, i)
    assert len(flush) == 3
    limit[0] = 2
    flush.put(3, None, 3)
    assert list(flush) == [3]


def test_clear_len_truthiness_and_values():
    cache = PinnedCache(4)
    assert not cache and len(cache) == 0 and list(cache.values()) == [] and "a" not in cache
    src = torch.zeros(2)
    cache.put("a", src, False)                          # a stored False is a value, not a miss
    cache.put("b", [src, src], None)
    assert cache and len(cache) == 2 and "a" in cache and cache.get("a") is False
    assert list(cache.values()) == [False, None], "values() yields the stored values, not the pins"
    snapshot = list(cache.values())
    cache.clear()
    assert not cache and len(cache) == 0 and cache.get("a") is None and snapshot == [False, None]


def test_graph_entry_is_captured_once_it_has_a_graph():
    ent = GraphEntry(pins=[1])
    assert not ent.captured and (ent.x, ent.t, ent.out, ent.graph) == (None, None, None, None)
    ent.graph = object()
    assert ent.captured


def test_assigning_none_to_a_cache_of_the_wrapper_clears_it_and_keeps_the_cache():
    from ccedit_amd.network import OpenAIWrapperControlLDM3DTV2V
    w = OpenAIWrapperControlLDM3DTV2V(torch.nn.Identity())
    cache = w._twin_val
    cache.put("k", None, True)
    w._twin_val = None                                  # the earlier spelling of a clear
    assert w._twin_val is cache and not cache
    w.reset_caches()
    w.frame_shard = None                                # every other attribute is set as usual
    assert w.__dict__["frame_shard"] is None
