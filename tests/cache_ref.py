"""A worst-case allocator for the prepared-weight caches of models/fused.py (plain Python, no GPU needed).

`fused.cached()` and `fused.folded_conv_bn()` key their entries on (data_ptr, _version) of the tensors an entry was built from.
Some of those tensors are themselves cache values (a `torch.cat` of two weights, a folded matrix, its slices): freshly allocated,
version 0.  Whether a re-derived tensor lands on the address of the one it replaces is up to the allocator, so a test that relies
on the real allocator tests its luck.  `worst_case_allocator` removes the luck: under it EVERY rebuilt cache value reappears in
the storage of its predecessor — same tensor objects, same data_ptr, same _version, new contents.  A dependent entry keyed on
such a value therefore always sees a matching key after its parent was rebuilt; it is served stale unless the product guards
against exactly that (keys on the source parameters, or drops dependents when the parent is rebuilt — the wrapper does not care).
"""
from __future__ import annotations

import contextlib

import torch

from adverse_weather_semantic_segmentation_robustness_benchmark_amd.models import fused

PREFIX = "_awseg_"
TENSOR_ATTRS = ("_awseg_exp", "_awseg_bf16")        # what the builders hang on the tensors they return
_DIFFERENT = object()


def _same_structure(old, new) -> bool:
    if isinstance(old, torch.Tensor) or isinstance(new, torch.Tensor):
        return (isinstance(old, torch.Tensor) and isinstance(new, torch.Tensor) and old is not new
                and old.shape == new.shape and old.dtype == new.dtype and old.device == new.device
                and old.stride() == new.stride() and old.storage_offset() == new.storage_offset()
                and old.untyped_storage().nbytes() == new.untyped_storage().nbytes()
                and old.untyped_storage().data_ptr() != new.untyped_storage().data_ptr())
    if isinstance(old, (tuple, list)) or isinstance(new, (tuple, list)):
        return (type(old) is type(new) and len(old) == len(new) and all(_same_structure(o, n) for o, n in zip(old, new)))
    return type(old) is type(new)


def _bytes_of(t: torch.Tensor) -> torch.Tensor:
    """The whole storage under `t` as a flat uint8 tensor with a version counter of its own (a split-operand image is a view in
    front of a trailer that the kernels read: the trailer has to move with the image)."""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def _into_old(old, new):
    """New contents in the old tensor objects (structure already checked); plain Python leaves are taken from `new`."""
    if isinstance(old, torch.Tensor):
        ptr, ver = old.data_ptr(), old._version
        with torch.no_grad():
            _bytes_of(old).copy_(_bytes_of(new))
        for a in TENSOR_ATTRS:
            if hasattr(new, a):
                setattr(old, a, getattr(new, a))
            elif hasattr(old, a):
                delattr(old, a)
        assert (old.data_ptr(), old._version) == (ptr, ver), "the harness must not move what the caches key on"
        return old
    if isinstance(old, (tuple, list)):
        return type(old)(_into_old(o, n) for o, n in zip(old, new))
    return new


def _reuse(old_entry, new_entry):
    """(key, value...) of a rebuilt entry with the value living in its predecessor's storage, or _DIFFERENT."""
    old_val, new_val = tuple(old_entry[1:]), tuple(new_entry[1:])
    if not _same_structure(old_val, new_val):
        return _DIFFERENT
    return (new_entry[0],) + _into_old(old_val, new_val)


@contextlib.contextmanager
def worst_case_allocator(monkeypatch):
    """Inside the block every rebuild by fused.cached / fused.folded_conv_bn hands back the tensors of the entry it replaces.
    Call sites resolve both names through the module at call time (fused.py's own calls are module-global look-ups, deeplab.py
    and model.py write `fused.cached(...)`), so patching the module attributes reaches all of them.  Yields a dict of counters."""
    real_cached, real_fold = fused.cached, fused.folded_conv_bn
    seen = {"rebuilt": 0, "reused": 0}

    def cached(module, name, tensors, fn):
        attr = PREFIX + name
        old = getattr(module, attr, None)
        val = real_cached(module, name, tensors, fn)
        new = getattr(module, attr, None)
        if new is not old:
            seen["rebuilt"] += 1
            if old is not None and new is not None:
                entry = _reuse(old, new)
                if entry is not _DIFFERENT:
                    seen["reused"] += 1
                    setattr(module, attr, entry)
                    return entry[1]
        return val

    def folded_conv_bn(conv, bn):
        old = getattr(conv, PREFIX + "fold", None)
        w, shift = real_fold(conv, bn)
        new = getattr(conv, PREFIX + "fold", None)
        if new is not old:
            seen["rebuilt"] += 1
            if old is not None and new is not None:
                entry = _reuse(old, new)
                if entry is not _DIFFERENT:
                    seen["reused"] += 1
                    conv._awseg_fold = entry
                    return entry[1], entry[2]
        return w, shift

    with monkeypatch.context() as mp:
        mp.setattr(fused, "cached", cached)
        mp.setattr(fused, "folded_conv_bn", folded_conv_bn)
        yield seen


def drop_caches(model) -> None:
    """Forget every prepared-weight image on every sub-module (the product's own way out: fused.drop_prepared)."""
    fused.drop_prepared(model)
    assert not cache_names(model)


def cache_names(model) -> set:
    """The <name>s of the `_awseg_<name>` cache entries present anywhere in `model`."""
    return {k[len(PREFIX):] for m in model.modules() for k, v in vars(m).items()
            if k.startswith(PREFIX) and isinstance(v, tuple)}
