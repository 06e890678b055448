"""CPU: the producer-to-sole-reader hand-over state of an Act (ops.py) and the PackCache's checks on a repeated vector.
A lazy view -- the raw output of a convolution standing for relu(bn(.)) -- is refused by every accessor but the one its
deferred reader uses, and its map is handed out once."""
import pytest
import torch
import torch.nn as nn

from unet_zoo_amd import _lib as L
from unet_zoo_amd.engine import PackCache
from unet_zoo_amd.ops import Act


def _act():
    # small integers: every product and sum below is exact in fp32
    buf = torch.arange(-12, 12, dtype=torch.float32).reshape(6, 4).to(torch.bfloat16)
    return Act(buf, 0, 4, 1, 2, 3)


def _lazy():
    a = _act()
    # 1 + 2^-10 times a bf16 value needs more mantissa bits than bf16 has: the result IS rounded
    a.lazy = (torch.tensor([0.5, 2.0, -1.0, 1.0 + 2.0 ** -10]), torch.tensor([3.0, -1.0, 0.0, 0.0]))
    return a


def test_fresh_act_hands_nothing_over():
    a = _act()
    assert a.lazy is None and a.bn_src is None and a.bn_partials is None and a.colsums is None
    assert a.ptr() == a.raw_ptr() == a.buf.data_ptr()
    assert a.window(1, 2).ptr() == a.buf.data_ptr() + 2 and a.rows(2, 1, 2, 2).P == 4
    assert a.take_lazy() is None and a.take_lazy() is None      # a real tensor has any number of readers


def test_lazy_act_is_refused_by_the_plain_accessors():
    a = _lazy()
    with pytest.raises(AssertionError):
        a.ptr()
    with pytest.raises(AssertionError):
        a.window(0, 2)
    with pytest.raises(AssertionError):
        a.rows(0, 1, 1, 3)
    assert a.raw_ptr() == a.buf.data_ptr()
    full = _lazy()
    full.parts = [_act()]
    with pytest.raises(AssertionError):
        full.add_grad(_act())


def test_lazy_dense_is_the_tensor_the_view_stands_for():
    a = _lazy()
    scale, shift = a.lazy
    raw = a.buf.double()
    want = torch.relu(raw * scale.double() + shift.double()).to(torch.bfloat16).float()     # exact, then ONE rounding
    got = a.dense()
    assert got.shape == (1, 4, 2, 3) and got.dtype == torch.float32
    assert torch.equal(got, want.reshape(1, 2, 3, 4).permute(0, 3, 1, 2))
    assert not torch.equal(want, torch.relu(raw * scale.double() + shift.double()).float())  # (the rounding was exercised)


def test_lazy_map_is_taken_once():
    a = _lazy()
    m = a.take_lazy()
    assert m is a.lazy and a.lazy is not None       # still lazy for everybody else
    with pytest.raises(AssertionError):
        a.take_lazy()
    with pytest.raises(AssertionError):
        a.ptr()


def test_pack_cache_repeated_vector_wants_contiguous_fp32():
    c = PackCache()
    p = nn.Parameter(torch.tensor([1.0, -2.0, 3.5]))
    got = c.get(p, L.PACK_VEC_REPEAT, 4, torch.bfloat16)
    assert got.dtype == torch.float32 and torch.equal(got, torch.tensor([1.0, -2.0, 3.5] * 4))
    assert c.get(p, L.PACK_VEC_REPEAT, 4, torch.bfloat16) is got
    with pytest.raises(AssertionError):
        c.get(nn.Parameter(p.detach().to(torch.bfloat16)), L.PACK_VEC_REPEAT, 4, torch.bfloat16)
    with pytest.raises(AssertionError):
        c.get(nn.Parameter(torch.arange(6.0)[::2]), L.PACK_VEC_REPEAT, 4, torch.bfloat16)
