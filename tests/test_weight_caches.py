"""The prepared-weight caches of models/fused.py on CPU tensors: the contract of `cached` / `folded_conv_bn` (what makes an entry
rebuild, what does not), the worst-case allocator of tests/cache_ref.py checked against a toy it must catch, and the four
parent -> dependent pairs of the eval executors (an entry keyed on another entry's tensor) driven through the real `cached` with
stand-in builders.  The executors themselves run on the GPU: tests/test_gpu_weight_caches.py."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models import fused
from tests import cache_ref


class Toy(nn.Module):
    """Two Linear layers whose weights are packed into one matrix (the parent entry) and an image of that matrix (the dependent
    entry), looked up the way the executors do it: through the `fused` module, parent first."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = nn.Linear(6, 4), nn.Linear(6, 4)
        self.built = {"pack": 0, "on_parent": 0, "on_sources": 0}

    def pack(self):
        def build():
            self.built["pack"] += 1
            return torch.cat([self.a.weight, self.b.weight]).contiguous()
        return fused.cached(self, "toy_pack", [self.a.weight, self.b.weight], build)

    def _image(self, which, pack):
        self.built[which] += 1
        return pack.detach() * 2.0

    def image_keyed_on_parent(self):
        pack = self.pack()
        return fused.cached(self, "toy_on_parent", (pack,), lambda: self._image("on_parent", pack))

    def image_keyed_on_sources(self):
        pack = self.pack()
        return fused.cached(self, "toy_on_sources", [self.a.weight, self.b.weight], lambda: self._image("on_sources", pack))

    def want(self):
        return torch.cat([self.a.weight, self.b.weight]).detach() * 2.0


def test_worst_case_allocator_serves_a_parent_keyed_dependent_stale(monkeypatch):
    """The guard's guard: under the wrapper the rebuilt parent follows the update in its predecessor's storage, so an entry keyed on
    the parent's tensor is served stale and its builder is not called again; an entry keyed on the parameters follows."""
    toy = Toy()
    with cache_ref.worst_case_allocator(monkeypatch) as seen:
        pack0 = toy.pack()
        assert torch.equal(toy.image_keyed_on_parent(), toy.want()) and torch.equal(toy.image_keyed_on_sources(), toy.want())
        where = (pack0.data_ptr(), pack0._version)
        with torch.no_grad():
            toy.a.weight.mul_(0.5)
        pack1 = toy.pack()
        assert toy.built["pack"] == 2 and seen["reused"] >= 1
        assert pack1 is pack0 and (pack1.data_ptr(), pack1._version) == where          # same key ...
        assert torch.equal(pack1, torch.cat([toy.a.weight, toy.b.weight]))              # ... new contents
        assert not torch.equal(toy.image_keyed_on_parent(), toy.want()) and toy.built["on_parent"] == 1      # stale, builder not called
        assert torch.equal(toy.image_keyed_on_sources(), toy.want()) and toy.built["on_sources"] == 2
    assert fused.cached.__module__ == fused.__name__                                    # the patch is gone with the block


def test_worst_case_allocator_carries_tensor_attributes_and_whole_storage(monkeypatch):
    """What the builders hang on a tensor (`_awseg_exp`, `_awseg_bf16`) and the bytes behind a view (a split-operand image sits in
    front of a trailer the kernels read) move with the rebuilt value; a value of another shape is left to the real behaviour."""
    m = nn.Linear(4, 4)
    n = [0]

    def build():
        n[0] += 1
        buf = torch.full((10,), float(n[0]))
        img = buf[:8].view(2, 4)
        img._awseg_exp = n[0]
        if n[0] == 1:
            img._awseg_bf16 = True
        return img
    with cache_ref.worst_case_allocator(monkeypatch):
        a = fused.cached(m, "toy_img", [m.weight], build)
        with torch.no_grad():
            m.weight.add_(1.0)
        b = fused.cached(m, "toy_img", [m.weight], build)
        assert b is a and b._awseg_exp == 2 and not hasattr(b, "_awseg_bf16")
        assert torch.equal(cache_ref._bytes_of(b).view(torch.float32), torch.full((10,), 2.0))          # trailer included
        with torch.no_grad():
            m.weight.add_(1.0)
        c = fused.cached(m, "toy_img", [m.weight], lambda: torch.zeros(3))
        assert c is not a and c.shape == (3,)


def test_cached_rebuilds_on_every_visible_update_and_only_then():
    toy = Toy()
    toy.pack(); toy.pack()
    assert toy.built["pack"] == 1                                           # unchanged module: one build
    with torch.no_grad():
        toy.b.weight.add_(0.25)                                             # in-place under no_grad (what an optimiser step does)
    assert torch.equal(toy.pack(), torch.cat([toy.a.weight, toy.b.weight])) and toy.built["pack"] == 2
    toy.pack()
    assert toy.built["pack"] == 2
    other = {k: v * 0.5 + 0.1 for k, v in toy.state_dict().items()}
    toy.load_state_dict(other)                                              # early stopping's path: copy_ into the parameters
    assert torch.equal(toy.pack(), torch.cat([other["a.weight"], other["b.weight"]])) and toy.built["pack"] == 3
    toy.double()                                                            # module.to(dtype): the storage is replaced ...
    with torch.no_grad():
        toy.a.weight.mul_(3.0)
    toy.float()                                                             # ... and replaced again
    assert torch.equal(toy.pack(), torch.cat([toy.a.weight, toy.b.weight])) and toy.built["pack"] == 4
    with torch.no_grad():
        for p in toy.parameters():
            p.data = p.data * 0.5                                           # a new storage beside the old one: another address
    assert torch.equal(toy.pack(), torch.cat([toy.a.weight, toy.b.weight])) and toy.built["pack"] == 5
    toy.pack()
    assert toy.built["pack"] == 5


def _conv_bn(seed=0, bias=True):
    torch.manual_seed(seed)
    conv, bn = nn.Conv2d(4, 8, 3, padding=1, bias=bias), nn.BatchNorm2d(8)
    with torch.no_grad():
        bn.running_var.copy_(torch.rand(8) + 0.5); bn.running_mean.copy_(torch.randn(8) * 0.1)
        bn.weight.copy_(torch.rand(8) + 0.5); bn.bias.copy_(torch.randn(8) * 0.1)
    return conv.eval(), bn.eval()


def _folded_matches_modules(conv, bn, x):
    w, shift = fused.folded_conv_bn(conv, bn)
    with torch.no_grad():
        got = F.conv2d(x, w, None, conv.stride, conv.padding) + shift.view(1, -1, 1, 1)
        ref = bn(conv(x))
    return (got - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("bias", [True, False])
def test_folded_conv_bn_follows_each_of_its_sources(bias):
    conv, bn = _conv_bn(1, bias)
    x = torch.randn(2, 4, 9, 7)
    assert _folded_matches_modules(conv, bn, x)
    first = conv._awseg_fold
    assert _folded_matches_modules(conv, bn, x) and conv._awseg_fold is first               # unchanged: not rebuilt
    sources = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var] + ([conv.bias] if bias else [])
    for t in sources:
        before = conv._awseg_fold
        with torch.no_grad():
            if t is bn.running_var:
                t.mul_(0.75).add_(0.05 * torch.rand_like(t))
            else:
                t.mul_(0.75).add_(0.05 * torch.randn_like(t))
        assert _folded_matches_modules(conv, bn, x) and conv._awseg_fold is not before
    other = copy.deepcopy(bn.state_dict())
    other["running_mean"] += 0.3
    bn.load_state_dict(other)
    assert _folded_matches_modules(conv, bn, x)


def test_data_writes_are_invisible_and_drop_prepared_is_the_way_out():
    """Documented blind spot: a write through `.data` does not move `_version` (tests' calibrate_bn sets BatchNorm weights that
    way, before the first forward), so the keys cannot see it.  `fused.drop_prepared(model)` forgets every prepared image."""
    conv, bn = _conv_bn(2)
    seq = nn.Sequential(conv, bn)
    x = torch.randn(1, 4, 5, 5)
    assert _folded_matches_modules(conv, bn, x)
    v = bn.weight._version
    bn.weight.data.mul_(0.5)
    assert bn.weight._version == v                                           # the blind spot itself
    assert not _folded_matches_modules(conv, bn, x)                          # stale: the old fold is served
    assert cache_ref.cache_names(seq) == {"fold"}
    fused.drop_prepared(seq)
    assert cache_ref.cache_names(seq) == set() and not hasattr(conv, "_awseg_fold")
    assert _folded_matches_modules(conv, bn, x)                              # follows
    toy = Toy()
    toy.image_keyed_on_sources()
    toy.a.weight.data.add_(1.0)
    assert not torch.equal(toy.image_keyed_on_sources(), toy.want())
    cache_ref.drop_caches(toy)
    assert torch.equal(toy.image_keyed_on_sources(), toy.want())


# The executors' four entries that are keyed on ANOTHER ENTRY's tensor, looked up as fused.py / deeplab.py do it (parent, then
# dependent on the same module), with a stand-in builder for the split-operand image (the real one is a HIP kernel).
def _pair_patch(mod):
    conv, bn = mod
    w2, _ = fused.cached(conv, "patch", [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var],
                         lambda: (fused.patch_weights(conv, bn.weight * torch.rsqrt(bn.running_var + bn.eps)), bn.bias.detach().clone()))
    return w2, fused.cached(conv, "wsplit_small", (w2,), lambda: w2.detach() * 2.0)


def _pair_kv(mod):
    conv, bn = mod
    wkv = fused.cached(conv, "kvpack", [conv.weight, bn.weight], lambda: torch.cat([conv.weight.flatten(), bn.weight]).contiguous())
    return wkv, fused.cached(conv, "kvsplit", (wkv,), lambda: wkv.detach() * 2.0)


def _pair_proj(mod):
    conv, bn = mod
    parts = fused.cached(conv, "proj_fold1", (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var),
                         lambda: [(conv.weight[:, i] * bn.weight.view(-1, 1, 1)).contiguous() for i in range(4)])
    cat = torch.cat(parts, dim=1)
    return cat, fused.cached(conv, "proj_pieces", tuple(parts), lambda: cat.detach() * 2.0)


def _pair_stem(mod):
    conv, bn = mod
    w, _ = fused.folded_conv_bn(conv, bn)
    return w, fused.cached(conv, "stemrows", [w], lambda: w.detach() * 2.0)


@pytest.mark.parametrize("worst_case", [False, True], ids=["real_allocator", "worst_case_allocator"])
@pytest.mark.parametrize("pair", [_pair_patch, _pair_kv, _pair_proj, _pair_stem], ids=["wsplit_small", "kvsplit", "proj_pieces", "stemrows"])
def test_entries_keyed_on_another_entry_follow_its_sources(pair, worst_case, monkeypatch):
    """Two updates with a look-up after each (and a third look-up that must not rebuild): the dependent is the image of the parent as
    it is NOW, whether or not the rebuilt parent sits where the old one sat."""
    mod = _conv_bn(3)
    with (cache_ref.worst_case_allocator(monkeypatch) if worst_case else monkeypatch.context()):
        parent, dep = pair(mod)
        assert torch.equal(dep, parent * 2.0)
        for _ in range(2):
            with torch.no_grad():
                mod[0].weight.mul_(0.75).add_(0.05 * torch.randn_like(mod[0].weight))
                mod[1].weight.mul_(0.75).add_(0.05 * torch.randn_like(mod[1].weight))
            parent, dep = pair(mod)
            assert torch.equal(dep, parent.detach() * 2.0)
        again, dep2 = pair(mod)
        assert dep2 is dep
