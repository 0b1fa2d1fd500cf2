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


# -- the second payload byte: 0xFF is a legal value of the integer outputs ------------------------------
INT_POISON = [(torch.int64, -1, 0), (torch.int32, -1, 0), (torch.uint8, 255, 0), (torch.bool, True, False)]


@pytest.mark.parametrize('dtype, under_ff, under_00', INT_POISON)
def test_integer_poison_values_under_both_payloads(dtype, under_ff, under_00):
    assert GuardedArena(G).payload == 0xFF               # the default: existing behaviour
    for payload, want in ((0xFF, under_ff), (0x00, under_00)):
        a = GuardedArena(G, payload=payload)
        t = a.alloc((3, 7), 'cpu', dtype)
        assert t.dtype == dtype and bool((t == want).all()), (dtype, payload, t)
        buf, off, nbytes = _buffer_of(a)
        assert bool((buf[off:off + nbytes] == payload).all())
        # the bands stay 0xFF whatever the payload byte is
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + nbytes:] == 0xFF).all())
        assert a.check() == 1


def test_between_the_payloads_every_unwritten_element_differs():
    """whatever an integer output is expected to hold, it is not both 0xFF.. and 0x00.."""
    for dtype, under_ff, under_00 in INT_POISON:
        assert under_ff != under_00
        for expected in (under_ff, under_00, 1 if dtype is not torch.bool else True):
            seen = [GuardedArena(G, payload=p).alloc((1,), 'cpu', dtype)[0].item() for p in (0xFF, 0x00)]
            assert any(v != expected for v in seen), (dtype, expected, seen)


@pytest.mark.parametrize('payload', [0xFF, 0x00])
def test_one_byte_past_a_uint8_payload_is_reported_under_either_payload(monkeypatch, payload):
    from emsanet_amd import functional as Fn
    a = GuardedArena(G, payload=payload)
    install(monkeypatch, a)

    def fake_wrapper():
        return Fn._empty((5, 3), 'cpu', torch.uint8)
    t = fake_wrapper()
    buf, off, nbytes = _buffer_of(a)
    assert nbytes == 15
    buf[off:off + nbytes + 1] = 7                        # "the kernel" writes 16 labels into 15
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert re.search(r'test_guard\.py:fake_wrapper:\d+ shape \(5, 3\) torch\.uint8: rear band damaged, '
                     r'first byte at offset 0 \(payload end \+ 0\), 1 bytes', msg), msg
    assert 'front band' not in msg
    del t


@pytest.mark.parametrize('payload', [0xFF, 0x00])
@pytest.mark.parametrize('dtype', [torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool])
def test_zeros_is_zero_under_either_payload(payload, dtype):
    a = GuardedArena(G, payload=payload)
    z = a.zeros((4, 9), 'cpu', dtype)
    assert z.dtype == dtype and bool((z == 0).all())
    buf, off, nbytes = _buffer_of(a)
    assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + nbytes:] == 0xFF).all())
    assert a.check() == 1


def test_put_is_the_same_under_either_payload():
    for payload in (0xFF, 0x00):
        a = GuardedArena(G, payload=payload)
        v = torch.arange(11, dtype=torch.uint8)
        g = a.put(v)
        assert torch.equal(g, v)
        buf, off, nbytes = _buffer_of(a)
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + nbytes:] == 0xFF).all())
        a.check()


# -- twins: the 0x00 run of a module whose tests keep their names ----------------------------------------
_TWIN_SOURCE = '''
import pytest
from os.path import join as test_imported            # not of this module: no twin

def helper():
    return 0

@pytest.mark.parametrize('a', [1, 2])
@pytest.mark.usefixtures('tmp_path')
def test_one(a, b=3, *, c=4):
    """doc"""
    return a + b + c

def test_training_step_on_an_augmented_batch():       # opted out in guard.OPT_OUT
    return 0
'''


def test_second_payload_adds_a_twin_per_test_with_its_marks():
    import guard
    ns = {'__file__': '/somewhere/test_augment_gpu.py', '__name__': 'twin_source'}
    exec(_TWIN_SOURCE, ns)
    before = set(ns)
    assert guard.second_payload(ns) == ['test_one_poison00']
    assert set(ns) - before == {'test_one_poison00'}
    one, twin = ns['test_one'], ns['test_one_poison00']
    assert twin is not one and twin.__name__ == twin.__qualname__ == 'test_one_poison00'
    assert twin.__code__ is one.__code__ and twin.__doc__ == 'doc' and twin(1) == one(1) == 8
    assert [m.name for m in twin.pytestmark] == [m.name for m in one.pytestmark] == ['usefixtures', 'parametrize']
    assert twin.pytestmark is not one.pytestmark
    assert guard.second_payload(ns) == []                # twins get no twins


class _Node:
    def __init__(self, name):
        self.fspath, self.originalname, self.name = '/somewhere/test_augment_gpu.py', name, name + '[x]'


class _Request:
    def __init__(self, name):
        self.node = _Node(name)


@pytest.mark.parametrize('name, payload', [('test_one', 0xFF), ('test_one_poison00', 0x00)])
def test_fixture_gives_a_twin_the_zero_payload(monkeypatch, capsys, name, payload):
    import guard
    from emsanet_amd import functional as Fn
    gen = guard._guarded(_Request(name), monkeypatch, 0xFF)
    arena = next(gen)
    assert arena.payload == payload and guard._ACTIVE[-1] is arena
    want = {0xFF: -1, 0x00: 0}[payload]
    assert bool((Fn._empty((5,), 'cpu', torch.int32) == want).all())
    assert bool((guard.put(torch.arange(3)) == torch.arange(3)).all()) and guard.check() == 2
    with pytest.raises(StopIteration):
        next(gen)
    assert arena not in guard._ACTIVE and 'GUARD_COUNT test_augment_gpu.py' in capsys.readouterr().out


@pytest.mark.parametrize('suffix', ['', '_poison00'])
def test_fixture_leaves_an_opted_out_test_and_its_name_sake_alone(monkeypatch, suffix):
    import guard
    from emsanet_amd import functional as Fn
    gen = guard._guarded(_Request('test_training_step_on_an_augmented_batch' + suffix), monkeypatch, 0xFF)
    assert next(gen) is None and Fn._empty.__name__ == '_empty' and guard.put(None) is None
