"""wcache without a device: keys against a hand-built ema._Refresh, the registry against the package source, the clear,
eviction and pinning, the per-device layer views."""
import ast
import glob
import os
import re

import torch
import torch.nn as nn

from dkt_stereo_amd import conv, conv_c8, corr, ema, extractor, update, wcache
from dkt_stereo_amd.wcache import Key

PKG = os.path.dirname(os.path.abspath(wcache.__file__))
#: update.py tags the flow TENSOR with the features it was decoded from: no cache, and not on a layer
NOT_A_CACHE = {"_dkt_feat"}


def _refresh():
    R = ema._Refresh()
    R.vmap = {1000: (3, 4), 2000: (7, 9)}          # data_ptr -> (version before, after)
    R.gone = {3000}
    return R


def test_key_current_and_rekey():
    R = _refresh()
    # current: every named written tensor at its pre-update version; the unwritten 5000 and the absent bias do not matter
    k = Key(((1000, 3), None, (2000, 7), (5000, 1)), ((64, 64), "x"))
    assert R.current(k)
    assert R.rekey(k) == Key(((1000, 4), None, (2000, 9), (5000, 1)), ((64, 64), "x"))
    assert not R.current(R.rekey(k))               # (already at the new versions: stale for THIS update)
    # one stale tensor
    k = Key(((1000, 3), (2000, 6)))
    assert not R.current(k)
    assert R.rekey(k) == Key(((1000, 4), (2000, 6)))       # rekey moves exactly the pre-update versions
    # a tensor the fallback replaced
    assert not R.current(Key(((1000, 3), (3000, 0))))
    # no written tensor at all
    k = Key(((5000, 1), None), (2,))
    assert not R.current(k)
    assert R.rekey(k) == k
    # ints in `extra` that look like a written pointer and its version are not tensors
    k = Key(((5000, 1),), (1000, 3))
    assert not R.current(k) and R.rekey(k) == k
    k = Key(((2000, 7),), (1000, 3, (1000, 3)))
    assert R.current(k) and R.rekey(k) == Key(((2000, 9),), (1000, 3, (1000, 3)))


def test_key_of_reads_pointer_and_version():
    w, b = torch.zeros(3), torch.zeros(2)
    k = wcache.key_of(w, None, b, extra=(5,))
    assert k == Key(((w.data_ptr(), w._version), None, (b.data_ptr(), b._version)), (5,)) and hash(k) == hash(Key(*k))
    w.add_(1)
    assert wcache.key_of(w, None, b, extra=(5,)) != k
    assert wcache.key_of(w).extra == ()


def _cache_names_in_source():
    names = set()
    for path in glob.glob(os.path.join(PKG, "*.py")):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"_dkt_[a-z0-9_]+", node.value):
                names.add(node.value)
    return names


def test_registry_lists_every_cache_once():
    names = (_cache_names_in_source() - NOT_A_CACHE) | {"_zr_cache"}
    assert {"_dkt_packed", "_dkt_stem7", "_dkt_packed_c8", "_dkt_gru_c8", "_dkt_head_w", "_dkt_wt", "_dkt_folded",
            "_dkt_merged", "_dkt_view", "_dkt_scaled", "_dkt_grad", "_dkt_c8_buf"} <= names
    tables = (wcache.DERIVED_HOOKS, wcache.PACK_HOOKS, wcache.NOT_WEIGHTS)
    for name in sorted(names):
        assert sum(name in t for t in tables) == 1, name
    assert set().union(*tables) == names
    assert all(callable(f) for t in tables[:2] for f in t.values())
    assert (ema.DERIVED_HOOKS, ema.PACK_HOOKS, ema.NOT_WEIGHTS) == tables and ema.PACK_HOOKS is wcache.PACK_HOOKS \
        and ema.DERIVED_HOOKS is wcache.DERIVED_HOOKS and ema.NOT_WEIGHTS is wcache.NOT_WEIGHTS


class _Dummy:
    def __init__(self, key):
        self.key = key


def _entries(module, name):
    return [e for m in module.modules() for lst in (m.__dict__.get(name) or {}).values() for e in lst]


def test_clear_weight_cache_drops_every_registered_cache():
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.gru = update.ConvGRU(8, 8)
            self.conv, self.bn = nn.Conv2d(4, 6, 3, padding=1), nn.BatchNorm2d(6).eval()
            self.heads = nn.ModuleList([nn.Conv2d(4, 2, 3, padding=1), nn.Conv2d(4, 3, 3, padding=1)])
            self.one = nn.Conv2d(9, 5, 1)
    net = Net()
    net.gru._merged_zr()
    update._leading_outputs(net.conv, 2)
    update._scaled_layer(net.conv, 0.25)
    extractor._folded(net.conv, net.bn)
    extractor._merged_outputs(list(net.heads))
    corr._kmajor_weight(net.one)
    names = [*wcache.DERIVED_HOOKS, *wcache.PACK_HOOKS, *wcache.NOT_WEIGHTS]
    built = {"_zr_cache", "_dkt_view", "_dkt_scaled", "_dkt_folded", "_dkt_merged", "_dkt_wt"}
    for name in built:
        assert len(_entries(net, name)) == 1, name
    for name in names:
        if name not in built:
            wcache.store(net.one, name, "cpu", _Dummy(wcache.key_of(net.one.weight)))
    assert all(_entries(net, name) for name in names)
    conv.clear_weight_cache(net)
    for name in names:
        assert not _entries(net, name), name
    assert not net.gru._zr_cache
    assert torch.equal(net.gru._merged_zr().weight, torch.cat([net.gru.convz.weight, net.gru.convr.weight], 0))   # refills


def test_eviction_and_pinning():
    holder = nn.Identity()
    w = torch.zeros(4)
    es = [_Dummy(wcache.key_of(w, extra=(i,))) for i in range(4)]
    for e in es:
        assert wcache.store(holder, "_dkt_packed_c8", ("cpu", (4,)), e, keep=3) is e
    assert holder.__dict__["_dkt_packed_c8"][("cpu", (4,))] == es[1:]               # three stay, the newest last
    assert wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (4,)), es[0].key) is None
    assert wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (4,)), es[2].key) is es[2]
    assert wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (8,)), es[2].key) is None      # another slot
    w.add_(1)                                                                      # other tensors: evicts the rest
    new = _Dummy(wcache.key_of(w, extra=(0,)))
    wcache.store(holder, "_dkt_packed_c8", ("cpu", (4,)), new, keep=3)
    assert holder.__dict__["_dkt_packed_c8"][("cpu", (4,))] == [new]
    keep = []
    with conv_c8.pin_packs(keep):
        assert wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (4,)), new.key) is new
        assert wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (4,)), es[3].key) is None        # a miss pins nothing
        other = wcache.store(holder, "_dkt_gru_c8", ("cpu", (4,)), _Dummy(new.key), keep=3)
        wcache.store(holder, "_dkt_packed", ("cpu", (4,)), _Dummy(new.key))                      # not a C8S cache
    assert keep == [new, other]
    wcache.lookup(holder, "_dkt_packed_c8", ("cpu", (4,)), new.key)                # outside the block: nothing is pinned
    assert keep == [new, other]


def test_layer_views_are_cached_per_device_and_versioned():
    layer = nn.Conv2d(4, 6, 3, padding=1)
    v = update._leading_outputs(layer, 2)
    assert update._leading_outputs(layer, 2) is v and v.n == 2 and v.key.extra == (2,)
    assert list(layer.__dict__["_dkt_view"]) == ["cpu"]
    s = update._scaled_layer(layer, 0.25)
    assert update._scaled_layer(layer, 0.25) is s and s.scale == 0.25 and list(layer.__dict__["_dkt_scaled"]) == ["cpu"]
    with torch.no_grad():
        layer.weight.mul_(2)
    v2, s2 = update._leading_outputs(layer, 2), update._scaled_layer(layer, 0.25)
    assert v2 is not v and s2 is not s
    assert torch.equal(v2.weight, layer.weight[:2]) and torch.equal(s2.weight, layer.weight * 0.25)
