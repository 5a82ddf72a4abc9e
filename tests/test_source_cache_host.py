"""engine.SourceCache on the host (no library, no device): hit and miss, the pinned storage of the sources, the replaced
nn.Linear whose memory the allocator hands to its successor, and the empty copies."""
import copy
import gc
import pickle
import weakref

import pytest
import torch
import torch.nn as nn

from vit_ocm_wmsegmentation_amd.engine import SourceCache, signature


class _Counted:
    """make() of a cache site: a clone of the source, and how often it ran."""

    def __init__(self):
        self.calls = 0

    def __call__(self, t):
        def make():
            self.calls += 1
            return t.detach().clone()
        return make


def test_signature_is_address_and_version():
    a, b = torch.zeros(3), torch.zeros(3)
    assert signature((a, b)) == ((a.data_ptr(), a._version), (b.data_ptr(), b._version))
    assert signature(t for t in (a,)) == ((a.data_ptr(), a._version),)
    assert signature(()) == ()


def test_hit_on_unchanged_sources():
    cache, made = SourceCache(), _Counted()
    w, b = torch.randn(8, 8), torch.randn(8)
    first = cache.get("w", (w, b), made(w), "bf16")
    for _ in range(3):
        assert cache.get("w", (w, b), made(w), "bf16") is first
    assert made.calls == 1
    assert cache.peek("w") is first and cache.peek("other") is None
    assert cache.hit("w", signature((w, b)), "bf16") is first and cache.hit("w", signature((w,)), "bf16") is None


@pytest.mark.parametrize("change", ["add_", "data", "replaced", "extra"])
def test_miss_after_a_change(change):
    cache, made = SourceCache(), _Counted()
    p = nn.Parameter(torch.randn(16, 16))
    cache.get("w", (p,), made(p), "bf16")
    extra = "bf16"
    if change == "add_":
        with torch.no_grad():
            p.add_(1.0)
    elif change == "data":
        p.data = torch.randn(16, 16)
    elif change == "replaced":
        p = nn.Parameter(torch.randn(16, 16))
    else:
        extra = "fp32"
    got = cache.get("w", (p,), made(p), extra)
    assert made.calls == 2 and torch.equal(got, p.detach())
    assert cache.get("w", (p,), made(p), extra) is got and made.calls == 2


def test_entry_without_sources():
    """model._zeros: no sources, the device as the extra."""
    cache, made = SourceCache(), _Counted()
    z = cache.get(("zeros", 4), (), made(torch.zeros(4)), "cpu")
    assert cache.get(("zeros", 4), (), made(torch.zeros(4)), "cpu") is z and made.calls == 1
    assert cache.get(("zeros", 4), (), made(torch.zeros(4)), "meta") is not z and made.calls == 2


def _addresses(cache):
    return {t.data_ptr() for ent in cache._ent.values() for t in (*ent[3], ent[2]) if isinstance(t, torch.Tensor)}


def test_entry_pins_the_storage_of_its_sources():
    cache = SourceCache()
    src = torch.randn(384, 384)
    addr, storage = src.data_ptr(), weakref.ref(src.untyped_storage())
    cache.get("w", (src,), lambda: "derived")
    del src
    gc.collect()
    assert storage() is not None
    held = [torch.empty(384, 384) for _ in range(200)]  # all alive at once: none may be given the pinned address
    assert addr not in {t.data_ptr() for t in held}
    other = held[0]
    assert cache.get("w", (other,), lambda: "derived again") == "derived again"  # a miss replaces the entry: the pin goes
    gc.collect()
    assert storage() is None
    assert addr not in _addresses(cache) and other.data_ptr() in _addresses(cache)


def test_replaced_linear_never_reads_the_stale_copy():
    """A dropped nn.Linear(384, 384) and a fresh one: torch's CPU allocator hands the address on and both weights are at
    version 1, which a cache that keys on (data_ptr, _version) without holding its sources takes for a hit (197 of 200
    rounds with model._cached_operand before it kept them). Compared by value with the live weight."""
    cache, stale = SourceCache(), 0
    lin = nn.Linear(384, 384)
    for _ in range(200):
        w = lin.weight
        got = cache.get("w", (w,), lambda: w.detach().clone(), "bf16")
        stale += not torch.equal(got, lin.weight.detach())
        del w, got, lin
        gc.collect()
        lin = nn.Linear(384, 384)
    assert stale == 0


class _Holder(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(8, 8)
        self.__dict__["_cache"] = SourceCache()


def test_copies_and_pickles_are_empty():
    m = _Holder()
    m._cache.get("w", (m.lin.weight,), lambda: m.lin.weight.detach().clone())
    assert m._cache._ent
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert isinstance(twin._cache, SourceCache) and twin._cache is not m._cache and not twin._cache._ent
        assert torch.equal(twin.lin.weight, m.lin.weight)
    for twin in (copy.copy(m._cache), copy.deepcopy(m._cache), pickle.loads(pickle.dumps(m._cache))):
        assert isinstance(twin, SourceCache) and not twin._ent
    assert m._cache.peek("w") is not None  # the original keeps what it has


def test_package_modules_hold_source_caches():
    """The dict caches of the wrappers are SourceCache objects, so a deepcopy of a model carries no pins or derived copies."""
    import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
    from vit_ocm_wmsegmentation_amd import model as M
    mlp = vits.Mlp(64, 128)
    assert isinstance(mlp._w, SourceCache) and isinstance(copy.deepcopy(mlp)._w, SourceCache)
    vit = vits.vit_tiny(patch_size=16, num_classes=0)
    assert isinstance(vit._engines, SourceCache) and isinstance(vit._pos_cache, SourceCache)
    twin = copy.deepcopy(vit)
    assert twin._engines is not vit._engines and twin._pos_cache is not vit._pos_cache
    unet = M.build_unet()
    assert isinstance(unet._op_cache, SourceCache) and copy.deepcopy(unet)._op_cache is not unet._op_cache
