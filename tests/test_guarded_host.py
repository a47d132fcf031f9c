"""tests/guarded.py proves itself on the CPU: planted writes and reads -- plain torch ops through the arena buffer, inside the arena,
nothing faults -- must be reported for the right allocation and side; everything else must pass."""
import pytest
import torch

import guarded as GD
from guarded import GUARD, GuardViolation, guarded

CPU = torch.device("cpu")
SMALL = 4 << 20


def test_one_element_past_an_output_is_reported_for_that_allocation_and_side():
    with guarded(CPU, SMALL, check_on_exit=False) as g:
        first = torch.empty((3, 5), dtype=torch.float32, device=CPU)
        out = torch.empty((7, 9), dtype=torch.float32, device=CPU)
        last = torch.empty(11, dtype=torch.float32, device=CPU)
        assert g.violations() == []
        a = g.allocations[1]
        assert (a.shape, a.dtype, a.nbytes) == ((7, 9), torch.float32, 7 * 9 * 4)
        out.as_strided((1,), (1,), out.storage_offset() + out.numel()).view(torch.uint8)[0] = 1           # ONE byte of the element past the end
        found = g.violations()
    assert len(found) == 1, found
    msg = found[0]
    assert msg.startswith("after empty (7, 9) torch.float32") and "test_guarded_host.py" in msg, msg
    assert "1 guard bytes changed, the first at byte 0 past its end" in msg, msg
    del first, last


def test_one_element_before_an_output_is_reported():
    with pytest.raises(GuardViolation) as e:
        with guarded(CPU, SMALL) as g:
            torch.zeros(4, dtype=torch.float64, device=CPU)
            out = torch.empty((2, 6), dtype=torch.float16, device=CPU)
            off = g.allocations[1].offset
            g.arena[off - 2:off].view(torch.float16)[0] = 3.0                       # the element in front of out[0, 0]
    msg = str(e.value)
    assert "before empty (2, 6) torch.float16" in msg and "zeros" not in msg, msg
    assert "the first at byte -2 relative to its first byte" in msg or "the first at byte -1 relative" in msg, msg
    del out


def test_a_write_into_the_lead_in_is_reported():
    with guarded(CPU, SMALL, check_on_exit=False) as g:
        torch.empty(8, device=CPU)
        g.arena[17] = 0
        found = g.violations()
    assert len(found) == 1 and "outside every guard zone" in found[0] and "arena+17" in found[0], found


def test_a_read_one_element_past_a_placed_float_input_is_nan():
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for mis in (0, 4):
        with guarded(CPU, SMALL) as g:
            p = g.place(x, misalign=mis)
            assert p.data_ptr() % 256 == mis and torch.equal(p, x)
            inside = p.as_strided((12,), (1,), p.storage_offset()).sum()
            past = p.as_strided((13,), (1,), p.storage_offset()).sum()              # a ragged tile that reads one too many
            front = p.as_strided((13,), (1,), p.storage_offset() - 1).sum()
        assert float(inside) == 66.0 and torch.isnan(past) and torch.isnan(front)


def test_float64_operands_are_never_placed_off_their_element_size():
    with guarded(CPU, SMALL) as g:
        p = g.place(torch.ones(3, dtype=torch.float64), misalign=4)
        assert p.data_ptr() % 256 == 8


def test_an_index_operand_is_poisoned_inside_its_valid_range_only():
    idx = torch.tensor([4, 0, 2, 1], dtype=torch.int32)
    table = torch.arange(5, dtype=torch.float32) * 10
    with guarded(CPU, SMALL) as g:
        p = g.place(idx, index_fill=3)
        stray = p.as_strided((6,), (1,), p.storage_offset() - 1)                    # one entry on either side
        assert stray.tolist() == [3, 4, 0, 2, 1, 3]
        assert table[stray.long()].tolist() == [30.0, 40.0, 0.0, 20.0, 10.0, 30.0]  # changes the result, forms no wild address
        q = g.place(idx)
        assert q.as_strided((1,), (1,), q.storage_offset() + 4).item() == 0
    # a write into such a guard is still seen
    with guarded(CPU, SMALL, check_on_exit=False) as g:
        p = g.place(idx, index_fill=3)
        p.as_strided((1,), (1,), p.storage_offset() + 4)[0] = 2
        found = g.violations()
    assert len(found) == 1 and found[0].startswith("after place (4,) torch.int32"), found


def test_zeros_ones_and_full_fill_the_interior_only_and_empty_is_nan():
    with guarded(CPU, SMALL) as g:
        z = torch.zeros((5, 3), dtype=torch.float32, device=CPU)
        o = torch.ones(7, dtype=torch.int32, device=CPU)
        f = torch.full((2, 2), 2.5, device=CPU)
        fi = torch.full((3,), 7, device=CPU)
        e = torch.empty(6, dtype=torch.float16, device=CPU)
        e64 = torch.empty(2, dtype=torch.float64, device=CPU)
        e0 = torch.empty((), dtype=torch.float32, device=CPU)                       # zero-dimensional
        assert e0.shape == () and torch.isnan(e0)
        assert (z == 0).all() and (o == 1).all() and (f == 2.5).all() and f.dtype == torch.float32
        assert fi.dtype == torch.int64 and (fi == 7).all()
        assert torch.isnan(e).all() and torch.isnan(e64).all()
        for a in g.allocations:
            before = g.arena[a.offset - GUARD:a.offset]
            after = g.arena[a.offset + a.nbytes:a.offset + a.nbytes + GUARD]
            assert (before == 0xA5).all() and (after == 0xA5).all(), a
        assert g.counts == {"guarded": 7, "unguarded": 0}


def test_like_and_new_factories_and_their_spellings():
    with guarded(CPU, SMALL) as g:
        base = torch.empty(2, 3, dtype=torch.float64, device=CPU)                   # sizes as separate arguments
        got = [torch.empty_like(base), torch.zeros_like(base), base.new_empty((4,)), base.new_zeros(2, 2), base.new_full((3,), 1.5),
               torch.empty(size=(2, 2), device=CPU), torch.empty_like(base, dtype=torch.float32),
               base.new_empty((1,), dtype=torch.int16), torch.zeros(3, device=CPU, requires_grad=True)]
        assert [tuple(t.shape) for t in got] == [(2, 3), (2, 3), (4,), (2, 2), (3,), (2, 2), (2, 3), (1,), (3,)]
        assert [t.dtype for t in got[:5]] == [torch.float64] * 5 and got[6].dtype == torch.float32 and got[7].dtype == torch.int16
        assert (got[1] == 0).all() and (got[3] == 0).all() and (got[4] == 1.5).all() and got[8].requires_grad
        assert all(g._in_arena(t) for t in got) and g.counts == {"guarded": 10, "unguarded": 0}
        assert all(t.data_ptr() % 256 == 0 for t in got)


def test_a_workspace_of_n_bytes_has_its_guard_at_byte_n():
    for n in (1, 13, 1000, 4099):
        assert n % 16
        with guarded(CPU, SMALL, check_on_exit=False) as g:
            ws = torch.empty(n, dtype=torch.uint8, device=CPU)
            a = g.allocations[0]
            assert a.nbytes == n and ws.data_ptr() % 256 == 0
            assert int(g.arena[a.offset + n - 1]) == 0xFF and int(g.arena[a.offset + n]) == 0xA5
            g.arena[a.offset + n] = 0                                               # a query that returned one byte too few
            found = g.violations()
        assert len(found) == 1 and "the first at byte 0 past its end" in found[0], found


def test_zero_size_allocations():
    nothing = torch.empty(0, 3)
    with guarded(CPU, SMALL) as g:
        e = torch.empty((0, 4), device=CPU)
        z = torch.zeros(0, dtype=torch.uint8, device=CPU)
        p = g.place(nothing)
        assert e.shape == (0, 4) and z.numel() == 0 and p.shape == (0, 3) and g.counts["guarded"] == 3


def test_fall_through_allocations_are_counted():
    with guarded(CPU, SMALL) as g:
        a = torch.empty((2, 3, 4, 5), device=CPU, memory_format=torch.channels_last)
        b = torch.empty_like(torch.arange(6.0).reshape(2, 3).t())                   # would copy the transposed layout
        c = torch.empty(3, device="meta")
        d = torch.empty(4, device=CPU)
        assert [u.reason for u in g.unguarded] == ["a memory_format", "copies a non-contiguous layout", "another device"]
        assert [u.kind for u in g.unguarded] == ["empty", "empty_like", "empty"]
        assert all("test_guarded_host.py" in u.site for u in g.unguarded)
        assert g.counts == {"guarded": 1, "unguarded": 3} and len(g.unguarded_on_device()) == 2
        assert not g._in_arena(a) and not g._in_arena(b) and c.device.type == "meta" and g._in_arena(d)
        assert a.is_contiguous(memory_format=torch.channels_last) and b.stride() == (1, 3)


def test_arena_exhaustion_is_a_clear_error():
    with guarded(CPU, SMALL) as g:
        with pytest.raises(GD.ArenaExhausted, match="pass a larger arena_bytes"):
            torch.empty(SMALL, dtype=torch.uint8, device=CPU)
        torch.empty(16, device=CPU)          # the block is still usable


def test_tensors_cached_across_two_blocks_do_not_alias():
    cache = []
    with guarded(CPU, SMALL):
        cache.append(torch.zeros(64, dtype=torch.float32, device=CPU))
    with guarded(CPU, SMALL) as g:
        again = torch.empty(64, dtype=torch.float32, device=CPU)
        assert cache[0].untyped_storage().data_ptr() != again.untyped_storage().data_ptr()
        again.fill_(5.0)
        g.arena.fill_(0xA5)                  # even the whole new arena is not the old one
        g.shadow.fill_(0xA5)
    assert (cache[0] == 0).all()             # the first block's tensor is alive and untouched after its block
    cache[0].fill_(1.0)


def test_cached_device_buffers_of_the_package_are_made_anew_inside_the_block():
    """The workspaces, the scale scratch, the per-width constants and the maximum words: dropped on entry, created in the arena, one
    set of words per allocation (so its neighbours are guards), dropped again on exit."""
    from snvc_amd import ops
    ops._workspace  # noqa: B018  (the names this test relies on)
    before = ops.amax_word(CPU)
    ops._ONES_ZEROS[(3, CPU)] = (torch.ones(3), torch.zeros(3))
    ops._WORKSPACES["stale"] = torch.empty(4)
    size = ops._AMAX_POOL_WORDS
    with guarded(CPU, SMALL) as g:
        assert not ops._WORKSPACES and not ops._ONES_ZEROS and not ops._SCALE_SCRATCH and ops._AMAX_POOL_WORDS == 1
        w1, w2 = ops.amax_word(CPU), ops.amax_word(CPU)
        assert g._in_arena(w1) and g._in_arena(w2) and w1.shape == (ops.AMAX_SLOTS,) and not w1.any()
        assert [a.shape for a in g.allocations] == [(1, ops.AMAX_SLOTS)] * 2
        assert int(g.arena[g.allocations[0].offset + g.allocations[0].nbytes]) == 0xA5          # a guard, not the next set of words
        ones, zeros = ops._ones_zeros(5, CPU)
        assert g._in_arena(ones) and g._in_arena(zeros)
    assert ops._AMAX_POOL_WORDS == size and not ops._ONES_ZEROS and "pools" not in ops._AMAX_POOL.__dict__
    after = ops.amax_word(CPU)
    assert not g._in_arena(after) and not before.any()


def test_nothing_is_intercepted_outside_the_block():
    with guarded(CPU, SMALL) as g:
        pass
    t = torch.empty(4, device=CPU)
    assert g.counts == {"guarded": 0, "unguarded": 0} and g.arena is None and t.shape == (4,)


def test_place_results_puts_every_fresh_tensor_of_a_builder_into_the_arena():
    def builder():
        torch.manual_seed(3)
        x = torch.randn(2, 5) * 1.5
        idx = torch.tensor([2, 0, 1])
        return x, idx, x[:, 1:3], x.t().contiguous()

    plain = builder()
    with guarded(CPU, SMALL, place_results=True, misalign=4) as g:
        got = builder()
        assert all(g._in_arena(t) for t in got)
        assert got[0].data_ptr() % 256 == 4 and got[2].untyped_storage().data_ptr() == got[0].untyped_storage().data_ptr()
        assert got[1].data_ptr() % 256 == 8                                          # int64: the next multiple of its size
        assert torch.isnan(got[0].as_strided((1,), (1,), got[0].storage_offset() + 10)).all()                  # float guards are NaN
        assert got[1].as_strided((1,), (1,), got[1].storage_offset() + 3).item() == 0                          # index guards: the tensor's own minimum
        out = torch.empty(6, dtype=torch.float16)                                    # an output is the next kernel's operand: NaN around it
        ws = torch.empty(6, dtype=torch.uint8)
        assert torch.isnan(out.as_strided((8,), (1,), out.storage_offset() - 1)).all()
        assert ws.as_strided((1,), (1,), ws.storage_offset() + 6).item() == 0xA5
        assert g.violations() == []
        out.as_strided((1,), (1,), out.storage_offset() + 6).fill_(2.0)              # and a write into that guard is seen
        assert len(g.violations()) == 1 and g.violations()[0].startswith("after empty (6,) torch.float16")
        out.as_strided((1,), (1,), out.storage_offset() + 6).view(torch.uint8).fill_(0xFF)
    assert all(torch.equal(a, b) for a, b in zip(plain, got))


def test_place_results_keeps_the_autograd_graph():
    with guarded(CPU, SMALL, place_results=True) as g:
        w = torch.randn(4, requires_grad=True)
        assert w.is_leaf and g._in_arena(w)
        y = (w * 2.0).sum()
        y.backward()
    assert torch.equal(w.grad, torch.full((4,), 2.0))


def test_arena_tensors_have_version_counters_of_their_own():
    """Views of one buffer share its version counter: every write anywhere in the arena would void autograd's saved tensors and the
    tags of snvc_amd._derived."""
    with guarded(CPU, SMALL) as g:
        a = torch.empty(4, device=CPU)
        b = torch.zeros(4, device=CPU)
        p = g.place(torch.ones(3))
        va, vb, vp = a._version, b._version, p._version
        b.add_(1.0)
        torch.empty(4, device=CPU)          # fills its interior and is a write to the arena, too
        assert (a._version, b._version, p._version) == (va, vb + 1, vp)


def test_run_case_compares_every_factory_result_and_atomics_at_their_tolerance():
    from guarded import run_case
    noise = iter([0.0, 3e-7, 0.0, 3e-7, 0.0, 0.5])

    def case():
        torch.empty(5).copy_(torch.arange(5.0))                                      # deterministic: bit-compared
        torch.empty(3, dtype=torch.int32)[:2].fill_(-1)                              # a written -1 beside an unwritten element
        torch.empty(4).copy_(torch.ones(4) + next(noise))                            # atomics stand-in

    loose = (("atomics stand-in", 0.0, 1e-5),)
    g = run_case(case, CPU, arena_bytes=SMALL, loose=loose, what="within the tolerance")
    assert len(g.results) == 4                                                       # three empties and the ones
    with pytest.raises(AssertionError, match="bytes differ from the unguarded run"):
        run_case(case, CPU, arena_bytes=SMALL, what="bitwise")                       # the same difference without ``loose``
    with pytest.raises(AssertionError, match="differs from the unguarded run by 5.000e-01"):
        run_case(case, CPU, arena_bytes=SMALL, loose=loose, what="beyond the tolerance")
    runs = []

    def cached():
        runs.append(1)
        if len(runs) == 1:
            torch.zeros(2)
        torch.zeros(3)

    with pytest.raises(AssertionError, match="0 in the guarded run, 1 in the unguarded run"):
        run_case(cached, CPU, arena_bytes=SMALL, what="a buffer made in one run only")
