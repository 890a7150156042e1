"""The derived-weight cache (`synfmc_amd.derived`): a hit means these exact live tensors at this version.  CPU only, no built library."""
import gc
import types
import weakref

import torch

from synfmc_amd import derived as D


class Counter:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self):
        self.calls += 1
        return self.fn()


def test_hit_returns_the_identical_object_and_builds_once():
    holder, w = types.SimpleNamespace(), torch.randn(4, 6)
    build = Counter(lambda: (w.t().contiguous(), None))
    first = D.derived(holder, "_wt", [w], build)
    for _ in range(3):
        assert D.derived(holder, "_wt", [w], build) is first
    assert build.calls == 1 and torch.equal(first[0], w.t()) and first[1] is None


def test_build_runs_without_grad():
    holder, w = types.SimpleNamespace(), torch.randn(3, 3, requires_grad=True)
    with torch.enable_grad():
        assert not D.derived(holder, "_x", [w], lambda: w * 2).requires_grad
        assert not D.derived_on_owner(w, "_fmc_x", None, lambda: w * 2).requires_grad


def test_miss_on_an_in_place_write():
    holder, w, src = types.SimpleNamespace(), torch.ones(4), torch.full((4,), 3.0)
    build = Counter(lambda: w * 2)
    assert torch.equal(D.derived(holder, "_x", [w], build), torch.full((4,), 2.0))
    w.mul_(2.0)
    assert torch.equal(D.derived(holder, "_x", [w], build), torch.full((4,), 4.0)) and build.calls == 2
    w.copy_(src)
    assert torch.equal(D.derived(holder, "_x", [w], build), torch.full((4,), 6.0)) and build.calls == 3
    torch._C._increment_version([w])
    D.derived(holder, "_x", [w], build)
    assert build.calls == 4
    D.derived(holder, "_x", [w], build)
    assert build.calls == 4


def test_miss_on_replacement_and_the_entry_keeps_its_sources_alive():
    holder = types.SimpleNamespace()
    w = torch.randn(8, 8)
    ref = weakref.ref(w)
    first = D.derived(holder, "_x", [w], lambda: ref().clone())
    del w
    gc.collect()
    assert ref() is not None, "the entry must hold its sources: only then is an equal pointer the same live storage"
    # a new tensor with equal values, shape and version 0 (as after `p.data = ...` or a newly merged weight): while the entry holds
    # the old source, the new one cannot sit on its address, so the key differs and the old value is not handed out
    new = ref().clone()
    assert new._version == 0 and new.data_ptr() != ref().data_ptr()
    second = D.derived(holder, "_x", [new], lambda: new.clone())
    assert second is not first
    gc.collect()
    assert ref() is None, "the replaced entry lets its sources go"
    assert holder.__dict__["_x"][2][0] is new


def test_data_assignment_on_a_source_misses():
    holder, p = types.SimpleNamespace(), torch.nn.Parameter(torch.ones(4))
    build = Counter(lambda: p.detach() * 2)
    D.derived(holder, "_x", [p], build)
    p.data = torch.full((4,), 5.0)
    assert torch.equal(D.derived(holder, "_x", [p], build), torch.full((4,), 10.0)) and build.calls == 2


def test_none_sources_and_extra_are_part_of_the_key():
    holder, w, b = types.SimpleNamespace(), torch.randn(4), torch.randn(4)
    build = Counter(lambda: object())
    a = D.derived(holder, "_x", [w, None], build, extra=(1.0,))
    assert D.derived(holder, "_x", [w, None], build, extra=(1.0,)) is a and build.calls == 1
    assert D.derived(holder, "_x", [w, b], build, extra=(1.0,)) is not a and build.calls == 2
    D.derived(holder, "_x", [w, None], build, extra=(1.0,))
    assert build.calls == 3
    D.derived(holder, "_x", [w, None], build, extra=(0.5,))
    assert build.calls == 4


def test_layout_and_dtype_of_a_source_are_part_of_the_key():
    holder, w = types.SimpleNamespace(), torch.randn(4, 6)
    build = Counter(lambda: object())
    D.derived(holder, "_x", [w], build)
    for other in (w[1:], w.view(6, 4), w.t(), w.view(torch.int32)):
        D.derived(holder, "_x", [other], build)
    assert build.calls == 5


def test_tagged_entries_share_a_slot():
    holder, g, b = types.SimpleNamespace(), torch.randn(4), torch.randn(4)
    build = Counter(lambda: object())
    e0, e1 = D.derived(holder, "_c", [g], build, tag=0), D.derived(holder, "_c", [b], build, tag=1)
    assert D.derived(holder, "_c", [g], build, tag=0) is e0 and D.derived(holder, "_c", [b], build, tag=1) is e1 and build.calls == 2
    assert set(holder.__dict__["_c"]) == {0, 1}
    g.add_(1.0)
    assert D.derived(holder, "_c", [g], build, tag=0) is not e0 and D.derived(holder, "_c", [b], build, tag=1) is e1


def test_owner_form_fresh_views_share_one_entry():
    w = torch.nn.Parameter(torch.randn(8, 6, 1, 1))
    build = Counter(lambda: w.detach().view(8, 6).t().contiguous())
    first = D.derived_on_owner(w.view(8, 6), "_fmc_wt", None, build)
    assert D.derived_on_owner(w.view(8, 6), "_fmc_wt", None, build) is first and build.calls == 1


def test_owner_form_key():
    w = torch.randn(8, 6)
    build = Counter(lambda: object())
    seen = [D.derived_on_owner(v, "_fmc_x", tag, build) for tag, v in
            ((None, w), (None, w[2:]), (None, w[:6]), (None, w.view(6, 8)), (None, w.t()), (None, w.view(torch.int32)), ("other", w))]
    assert build.calls == 7 and len({id(s) for s in seen}) == 7
    assert D.derived_on_owner(w[2:], "_fmc_x", None, build) is seen[1] and D.derived_on_owner(w, "_fmc_x", "other", build) is seen[6]
    assert D.derived_on_owner(w, "_fmc_y", None, build) is not seen[0]          # another slot is another cache


def test_owner_form_a_write_to_the_owner_drops_every_entry():
    w = torch.randn(8, 6)
    build = Counter(lambda: object())
    D.derived_on_owner(w, "_fmc_x", None, build)
    D.derived_on_owner(w[2:], "_fmc_x", None, build)
    w[0].zero_()                                            # through a view: the owner's version moves with it
    assert len(w._fmc_x[1]) == 2
    D.derived_on_owner(w, "_fmc_x", None, build)
    assert len(w._fmc_x[1]) == 1 and build.calls == 3
    D.derived_on_owner(w[2:], "_fmc_x", None, build)
    assert build.calls == 4


def test_owner_form_data_assignment_drops_every_entry():
    p = torch.nn.Parameter(torch.ones(4, 4))
    assert torch.equal(D.derived_on_owner(p, "_fmc_x", None, lambda: p.detach() * 2), torch.full((4, 4), 2.0))
    v = p._version
    p.data = torch.full((4, 4), 3.0)
    assert p._version == v                                  # (the version does not see it: the storage pointer does)
    assert torch.equal(D.derived_on_owner(p, "_fmc_x", None, lambda: p.detach() * 2), torch.full((4, 4), 6.0))


def test_owner_form_does_not_keep_the_owner_alive():
    gc.collect()
    gc.disable()                                            # no cycle pass: only reference counts may free the owner
    try:
        w = torch.randn(8, 6, 1, 1)
        ref = weakref.ref(w)
        view = w.view(8, 6)
        out = D.derived_on_owner(view, "_fmc_wt", None, lambda: view.t().contiguous())
        del w, view
        assert ref() is None, "the entry (or its build closure) holds a view of the owner: a cycle through the owner's attribute"
        assert out.shape == (6, 8)
    finally:
        gc.enable()


def test_owner_that_takes_no_attributes_builds_per_call():
    class NoAttr:                                           # what the helper reads of a tensor, on an object without a __dict__
        __slots__ = ("_t",)
        _base = None

        def __init__(self, t):
            self._t = t

        def __getattr__(self, name):
            return getattr(self._t, name)
    t = NoAttr(torch.randn(4))
    build = Counter(lambda: object())
    assert D.derived_on_owner(t, "_fmc_x", None, build) is not D.derived_on_owner(t, "_fmc_x", None, build) and build.calls == 2


def test_drop_removes_only_the_named_slots():
    holder, w = types.SimpleNamespace(keep=1), torch.randn(4)
    for slot in ("_a", "_b", "_c"):
        D.derived(holder, slot, [w], lambda: object())
    D.drop(holder, "_a", "_c", "_never_there")
    assert set(holder.__dict__) == {"keep", "_b"}
