"""CPU tests of tests/memcheck.py: the guard bands report exactly the bytes changed outside the payload, and
assert_same_bits passes and fails exactly where torch.equal does, with a message that locates the difference."""
import pytest
import torch

from tests.memcheck import GUARD_BYTES, PATTERNS, Guarded, assert_same_bits, describe_difference


@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 255, 256, 1000, 65537])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_guarded_layout_and_fill(nbytes, pattern):
    g = Guarded(nbytes, "cpu", pattern)
    assert g.ptr % 256 == 0
    assert g.payload().numel() == nbytes and (nbytes == 0 or g.payload().data_ptr() == g.ptr)
    assert g.start >= GUARD_BYTES and g.total - g.end >= GUARD_BYTES
    assert g.check() is None
    if nbytes % 4 == 0 and nbytes:
        word = PATTERNS[pattern] - (2 ** 32 if PATTERNS[pattern] >= 2 ** 31 else 0)
        assert bool((g.payload(torch.int32) == word).all())


def test_pattern_meanings():
    g = Guarded(16, "cpu", "nan")
    assert bool(torch.isnan(g.payload(torch.float32)).all()) and bool(torch.isnan(g.payload(torch.bfloat16)).all())
    g.fill("ones")
    assert bool(torch.isnan(g.payload(torch.float32)).all()) and bool(torch.isnan(g.payload(torch.bfloat16)).all())
    g.fill("big")
    f, h = g.payload(torch.float32), g.payload(torch.bfloat16)
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(h).all())
    assert bool(torch.isinf(f + f).all()) and bool(torch.isinf((h.float() * 2).to(torch.bfloat16)).all())
    g.fill("unit")
    assert bool((g.payload(torch.bfloat16) == 1.0).all()) and abs(float(g.payload(torch.float32)[0]) - 1.0019) < 1e-4
    g.fill("zero")
    assert bool((g.payload(torch.int32) == 0).all())


@pytest.mark.parametrize("side,offset", [("front", -1), ("front", -GUARD_BYTES), ("back", 0), ("back", 5),
                                         ("back", GUARD_BYTES - 1)])
def test_check_reports_a_changed_guard_byte(side, offset):
    g = Guarded(1000, "cpu", "unit")
    raw = g._buf.view(torch.uint8)
    at = (g.start if side == "front" else g.end) + offset
    raw[at] ^= 0x10
    msg = g.check()
    assert msg is not None and f"{side} guard: 1 byte(s) changed at offsets {offset} .. {offset}" in msg
    assert ("back" if side == "front" else "front") not in msg
    raw[at] ^= 0x10
    assert g.check() is None


def test_check_ignores_payload_writes_and_reports_both_sides():
    g = Guarded(64, "cpu", "zero")
    g.payload().fill_(0xAB)  # every payload byte written: not a guard change
    g.fill_payload("big")
    assert g.check() is None
    raw = g._buf.view(torch.uint8)
    raw[g.start - 8:g.start - 2] = 1
    raw[g.end + 3] = 9
    raw[g.end + 40] = 9
    msg = g.check()
    assert "front guard: 6 byte(s) changed at offsets -8 .. -3" in msg
    assert "back guard: 2 byte(s) changed at offsets 3 .. 40" in msg


def test_check_compares_with_the_last_fill():
    g = Guarded(100, "cpu", "nan")
    g.fill("ones")
    assert g.check() is None
    g._buf.view(torch.uint8)[g.end + 1] = 0xFE
    assert "back guard: 1 byte(s)" in g.check()


def _pairs():
    nan = float("nan")
    yield torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0])
    yield torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.5])
    yield torch.tensor([nan, 2.0]), torch.tensor([nan, 2.0])  # NaN is unequal to NaN: torch.equal is False
    yield torch.tensor([nan, 2.0]), torch.tensor([1.0, 2.0])
    yield torch.tensor([0.0]), torch.tensor([-0.0])  # equal values, different bits: torch.equal is True
    yield torch.zeros(2, 3), torch.zeros(3, 2)
    yield torch.arange(6, dtype=torch.int32), torch.arange(6, dtype=torch.int32)
    yield torch.arange(6, dtype=torch.int32), torch.arange(6, dtype=torch.int32).flip(0)
    yield torch.ones(3), torch.ones(3, dtype=torch.int64)
    yield torch.ones(3, dtype=torch.bfloat16), torch.ones(3, dtype=torch.bfloat16) * 2
    yield torch.tensor(3.0), torch.tensor(4.0)


@pytest.mark.parametrize("k", range(11))
def test_assert_same_bits_agrees_with_torch_equal(k):
    a, b = list(_pairs())[k]
    if torch.equal(a, b):
        assert_same_bits(a, b, "pair")
    else:
        with pytest.raises(AssertionError):
            assert_same_bits(a, b, "pair")


def test_assert_same_bits_message_locates_the_difference():
    a = torch.rand(4, 3, 10, 10, generator=torch.Generator().manual_seed(0))
    b = a.clone()
    b[1, 2, 3, 7] += 0.5
    b[2, 0, 9, 4] = float("nan")
    b[1, 1, 5, 5] -= 0.25
    with pytest.raises(AssertionError) as e:
        assert_same_bits(a, b, "last attention", axes=("image", "head", "row", "col"))
    msg = str(e.value)
    assert msg.startswith("last attention: 3 of 1200 elements differ")
    assert "max |delta| 0.5 over 2 finite pairs" in msg
    assert "NaN count: 0 (first) vs 1 (second)" in msg
    assert "extents: image 1..2, head 0..2, row 3..9, col 4..7" in msg
    assert "(1, 1, 5, 5)" in msg and "(1, 2, 3, 7)" in msg and "(2, 0, 9, 4)" in msg


def test_describe_difference_lists_at_most_eight_indices_and_default_axis_names():
    a = torch.zeros(20, 5)
    b = a.clone()
    b[::2, 1] = 1.0
    msg = describe_difference(a, b, "x")
    assert "10 of 100 elements differ" in msg and "extents: dim0 0..18, dim1 1..1" in msg
    assert msg.count("vs 1.0") == 8
    assert "shapes differ" in describe_difference(torch.zeros(2), torch.zeros(3), "y")
