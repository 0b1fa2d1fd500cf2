"""The guarded allocator of tests/guard.py on device='cpu' with plain torch writes: what it must
catch (overrun after / before, a write at the very last guard byte), what it must let pass, and
what its report says."""
import re

import pytest
import torch

from guard import ALIGN, GUARD_BYTES, GuardedArena, GuardError, install

G = 512                    # a small band keeps these host tests quick; the logic does not depend on it
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int8, torch.int64, torch.float64]


def _buffer_of(arena, k=-1):
    buf, off, nbytes = arena._live[k][:3]
    return buf, off, nbytes


def test_default_guard_is_the_largest_workgroup_tile():
    # the fp32 accumulator tile of the tap-split launch on 256 x 128 (conv_h.hip) = twice the largest
    # output tile, 128 x 128 fp32 (conv_mfma.hip) = 256 x 128 16-bit (conv_h.hip)
    assert GUARD_BYTES == 256 * 128 * 4 == 2 * 128 * 128 * 4 == 2 * 256 * 128 * 2
    assert GuardedArena().guard_bytes == GUARD_BYTES


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(1,), (3,), (2, 5, 7, 3), (0,), (5, 1, 1, 40)])
def test_alloc_looks_like_torch_empty(shape, dtype):
    a = GuardedArena(G)
    t = a.alloc(shape, 'cpu', dtype)
    ref = torch.empty(shape, dtype=dtype)
    assert t.shape == ref.shape and t.dtype == dtype and t.stride() == ref.stride()
    assert t.is_contiguous() and t.device == ref.device
    assert t.data_ptr() % ALIGN == 0
    buf, off, nbytes = _buffer_of(a)
    assert nbytes == ref.numel() * ref.element_size()
    # flush: the front band ends where the payload starts, the rear band starts at its last byte + 1
    assert off >= G and (buf.data_ptr() + off) % ALIGN == 0
    assert t.data_ptr() == (buf.data_ptr() + off if nbytes else 0)       # (torch: empty -> null)
    assert buf.numel() >= off + nbytes + G
    assert bool((buf == 0xFF).all())
    assert a.check() == 1


def test_negative_dimension_is_refused_like_torch_empty():
    with pytest.raises(RuntimeError):
        torch.empty((3, -1, 4))
    with pytest.raises(RuntimeError):
        GuardedArena(G).alloc((3, -1, 4), 'cpu')


def test_poison_values():
    a = GuardedArena(G)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert bool(torch.isnan(a.alloc((7,), 'cpu', dtype)).all())
    assert bool((a.alloc((7,), 'cpu', torch.int8) == -1).all())          # valid pool taps: 0..8
    assert bool((a.alloc((7,), 'cpu', torch.int64) == -1).all())         # every mask bit set
    assert bool((a.alloc((7,), 'cpu', torch.int32) == -1).all())
    z = a.zeros((7,), 'cpu', torch.bfloat16)
    assert bool((z == 0).all())
    buf, off, nbytes = _buffer_of(a)
    assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + nbytes:] == 0xFF).all())
    a.check()


def test_unwritten_element_stays_nan():
    a = GuardedArena(G)
    t = a.alloc((4, 5), 'cpu')
    t.view(-1)[:19] = 1.0                                # "the kernel" forgets the last element
    assert not bool(torch.isfinite(t).all())
    assert bool(torch.isnan(t.view(-1)[19]))
    a.check()                                            # (the guards themselves are intact)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.int8, torch.int64])
def test_overrun_by_one_element_after(dtype):
    a = GuardedArena(G)
    t = a.alloc((3, 5), 'cpu', dtype)
    buf, off, nbytes = _buffer_of(a)
    esz = t.element_size()
    wide = buf[off:off + nbytes + esz].view(dtype)       # the payload and one element more
    wide.fill_(0)
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert 'rear band' in msg and 'offset 0 ' in msg and f'{esz} bytes' in msg
    assert 'front band' not in msg


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.int8, torch.int64])
def test_overrun_by_one_element_before(dtype):
    a = GuardedArena(G)
    t = a.alloc((6,), 'cpu', dtype)
    buf, off, nbytes = _buffer_of(a)
    esz = t.element_size()
    buf[off - esz:off + nbytes].view(dtype).fill_(0)
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert 'front band' in msg and f'offset -{esz} ' in msg and f'{esz} bytes' in msg
    assert 'rear band' not in msg


def test_write_at_the_last_and_first_guard_byte():
    for pos in ('last', 'first'):
        a = GuardedArena(G)
        a.alloc((10,), 'cpu', torch.int8)
        buf, off, nbytes = _buffer_of(a)
        buf[off + nbytes + G - 1 if pos == 'last' else off - G] = 0
        with pytest.raises(GuardError) as e:
            a.check()
        want = f'offset {G - 1} ' if pos == 'last' else f'offset -{G} '
        assert want in str(e.value) and '1 bytes' in str(e.value)
    # one byte further out is no longer ours to watch: the buffer ends within ALIGN bytes of the band
    assert buf.numel() <= 2 * G + nbytes + ALIGN


def test_only_the_damaged_allocation_is_named_and_buffers_are_released():
    a = GuardedArena(G)
    a.alloc((4,), 'cpu')
    b = a.alloc((9, 2), 'cpu', torch.float16)
    a.alloc((4,), 'cpu', torch.int64)
    buf, off, nbytes = _buffer_of(a, 1)
    buf[off + nbytes + 3] = 7
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert msg.count('band damaged') == 1 and '(9, 2)' in msg and 'float16' in msg and 'offset 3 ' in msg
    assert a.checked == 3 and a._live == []
    assert a.check() == 0                                # nothing left: a second check passes
    del b


def test_put_copies_flush_against_the_guards():
    a = GuardedArena(G)
    x = torch.randn(2, 5, 3, 4).permute(0, 3, 1, 2)      # logical NCHW, NHWC memory
    g = a.put(x)
    assert torch.equal(g, x) and g.shape == x.shape and g.stride() == x.stride()
    assert g.data_ptr() % ALIGN == 0
    buf, off, nbytes = _buffer_of(a)
    assert nbytes == x.numel() * 4
    assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + nbytes:] == 0xFF).all())
    v = torch.arange(10, dtype=torch.bfloat16)
    assert torch.equal(a.put(v), v)
    s = torch.randn(2, 3, 8)[..., :5]                    # a slice: placed as its dense copy
    gs = a.put(s)
    assert torch.equal(gs, s) and gs.is_contiguous()
    assert a.put(None) is None
    assert a.check() == 3


def test_wrappers_allocate_from_the_arena_and_ld_views_work(monkeypatch):
    from emsanet_amd import functional as Fn
    a = GuardedArena(G)
    install(monkeypatch, a)
    assert Fn._POISON is False or Fn._POISON is True     # untouched: the hook replaces the functions
    t = Fn.act_empty(2, 5, 3, 4, 'cpu', ld=8)
    assert t.shape == (2, 5, 3, 4) and Fn.ld_of(t) == 8 and bool(torch.isnan(t).all())
    d = Fn.act_empty(2, 8, 3, 4, 'cpu', dtype=torch.bfloat16)
    assert Fn.ld_of(d) == 8 and d.dtype == torch.bfloat16
    z = Fn.act_zeros(1, 3, 2, 2, 'cpu')
    assert Fn.ld_of(z) == 3 and bool((z == 0).all())
    e = Fn._empty(12, 'cpu')                             # (an int shape, as pack_weight passes it)
    assert e.shape == (12,)
    t[:] = 1.0                                           # writing the slice leaves columns 5..8 NaN
    wide = torch.as_strided(t, (2, 3, 4, 8), (96, 32, 8, 1))
    assert wide.shape == (2, 3, 4, 8) and bool(torch.isnan(wide[..., 5:]).all())
    assert bool((wide[..., :5] == 1).all())
    assert a.check() == 4


def test_failure_message_carries_call_site_side_and_offset(monkeypatch):
    from emsanet_amd import functional as Fn
    a = GuardedArena(G)
    install(monkeypatch, a)

    def fake_wrapper():
        return Fn.act_empty(1, 4, 2, 2, 'cpu')
    t = fake_wrapper()
    buf, off, nbytes = _buffer_of(a)
    buf[off + nbytes:off + nbytes + 16] = 0
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    # the allocation helpers are skipped: the site is their caller (no package frame on the stack
    # here, so the test's own)
    assert re.search(r'test_guard\.py:fake_wrapper:\d+ shape \(1, 2, 2, 4\) torch\.float32: rear band '
                     r'damaged, first byte at offset 0 \(payload end \+ 0\), 16 bytes', msg), msg
    del t


def test_call_site_names_the_wrapper_in_the_package(monkeypatch):
    """an allocation made inside emsanet_amd/ is attributed to the wrapper, not to act_empty"""
    from emsanet_amd import functional as Fn
    a = GuardedArena(G)
    install(monkeypatch, a)
    monkeypatch.setattr(Fn, 'check', lambda *args: None)
    monkeypatch.setattr(Fn, '_stream', lambda: None)

    class _Lib:
        def emsa_add_t(self, *args):
            return 0
    monkeypatch.setattr(Fn._lib, 'lib', lambda: _Lib())
    x = torch.zeros(1, 2, 2, 4).permute(0, 3, 1, 2)
    Fn.add(x, x)
    assert re.match(r'functional\.py:add:\d+$', a._live[0][3]), a._live[0][3]
    a.check()
