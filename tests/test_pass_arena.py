"""srganst.disc_graph.PassArena on the CPU: the storage contract the batched discriminator backward relies on, without a kernel -
every pass's part is a view of ONE allocation per tensor, the parts lie side by side in slot order, BatchNorm coefficients are
[slots, C] tables, one batch size per arena, and the all-slots record exists only once every slot has run."""
import pytest
import torch

from srganst import disc_graph
from srganst.disc_graph import PLAN, PassArena

B, C = 3, 4


def _fill(arena, slot):
    """What forward(..., arena=(arena, slot)) asks of the arena, in its order (tiny shapes); returns the parts by (name, li)."""
    like = torch.zeros(1)
    parts = {("x3", None): arena.part(slot, "x3", None, (B, 5, 5, 3), like)}
    for li, (_, bi, _) in enumerate(PLAN):
        parts["y", li] = arena.part(slot, "y", li, (B, 5, 5, C), like)
        if bi is not None:
            parts["bn", li] = arena.part(slot, "bn", li, (C,), like)
    parts["flat", None] = arena.part(slot, "flat", None, (B, 100), like)
    parts["h1", None] = arena.part(slot, "h1", None, (B, 7), like)
    arena.filled.add(slot)
    return parts


def _packs_of(wd, ws2):
    return disc_graph._Saved(None, [], None, None, 1, 0, wd, ws2)


def test_slot_parts_are_adjacent_views_of_one_allocation():
    arena = PassArena(2)
    p1, p0 = _fill(arena, 1), _fill(arena, 0)               # the engine's order: slot 1 first
    assert arena.B == B
    for key in p0:
        name, li = key
        if name == "bn":
            continue
        full = getattr(arena, name) if li is None else getattr(arena, name)[li]
        a, b = p0[key], p1[key]
        assert full.shape == (2 * B, *a.shape[1:]) and full.is_contiguous() and full.dtype == torch.float32
        assert a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
        assert a.data_ptr() == full.data_ptr()                                          # slot 0 starts the allocation ...
        assert b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()              # ... slot 1 begins where slot 0 ends
        assert a._base is full and b._base is full
        assert _fill(arena, 1)[key].data_ptr() == b.data_ptr()                          # asked again: the same storage
    a, b = p0["y", 2], p1["y", 2]
    a.fill_(1.0)
    b.fill_(2.0)
    assert torch.equal(arena.y[2], torch.cat([torch.full_like(a, 1.0), torch.full_like(b, 2.0)]))


def test_batchnorm_tables_are_slots_by_channels():
    arena = PassArena(2)
    p1, p0 = _fill(arena, 1), _fill(arena, 0)
    rec = arena.all_slots(_packs_of(None, None))
    for li, (_, bi, _) in enumerate(PLAN):
        r = rec.layers[li]
        if bi is None:
            assert arena.bn[li] is None and r.mean is None and r.rstd is None and r.scale is None and r.shift is None
            continue
        tables = (r.mean, r.rstd, r.scale, r.shift)
        for k, t in enumerate(tables):
            assert t.shape == (2, C) and t.is_contiguous()
            for slot, parts in ((0, p0), (1, p1)):
                row = parts["bn", li][k]
                assert row.shape == (C,) and row.is_contiguous() and row.data_ptr() == t[slot].data_ptr()
        ptrs = sorted(t.data_ptr() for t in tables)
        assert all(q - p >= 2 * C * 4 for p, q in zip(ptrs, ptrs[1:]))                  # four tables, none overlapping
        p1["bn", li][2].fill_(float(li))
        assert torch.equal(r.scale[1], torch.full((C,), float(li)))


def test_a_second_batch_size_is_refused():
    arena = PassArena(2)
    like = torch.zeros(1)
    arena.part(1, "x3", None, (B, 5, 5, 3), like)
    with pytest.raises(AssertionError):
        arena.part(0, "x3", None, (B + 1, 5, 5, 3), like)
    with pytest.raises(AssertionError):
        arena.part(0, "y", 0, (B - 1, 5, 5, C), like)
    assert arena.B == B and arena.y[0] is None


def test_filled_gates_the_all_slots_record():
    arena = PassArena(2)
    wd, ws2 = {"a": 1}, {"b": 2}
    with pytest.raises(AssertionError):
        arena.all_slots(_packs_of(wd, ws2))
    _fill(arena, 1)
    with pytest.raises(AssertionError):
        arena.all_slots(_packs_of(wd, ws2))
    _fill(arena, 0)
    rec = arena.all_slots(_packs_of(wd, ws2))
    assert rec.groups == 2 and rec.gB == B and rec.wd is wd and rec.ws2 is ws2
    assert rec.x3 is arena.x3 and rec.flat is arena.flat and rec.h1 is arena.h1
    assert [(r.ci, r.bi, r.stride) for r in rec.layers] == PLAN
    assert all(r.y is arena.y[li] for li, r in enumerate(rec.layers))
    x, kw = rec.input_of(0)
    assert x is rec.x3 and kw["in_scale"] is None and kw["in_shift"] is None and kw["in_act"] == 0
    for li in range(1, len(PLAN)):
        x, kw = rec.input_of(li)
        assert x is rec.layers[li - 1].y and kw["in_scale"] is rec.layers[li - 1].scale and kw["in_shift"] is rec.layers[li - 1].shift
