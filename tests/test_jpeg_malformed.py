"""CPU: malformed JPEG streams are refused by the host parser with a status, in the single-image
entry points and in their slot of a batch (whose other images decode as usual): an
over-subscribed Huffman table, a scan that names a Huffman table above 3, and a sampling
layout the device stage does not take (4:4:0) reported as unsupported."""
import numpy as np
import pytest

from jpeg_cases import FIXTURES, variants

OK, INVALID, UNSUPPORTED = 0, 1, 4


def _segment(data: bytes, marker: int) -> int:
    """offset of the first FF <marker> segment, walking the marker segments from SOI"""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        if data[pos + 1] == marker:
            return pos
        assert data[pos + 1] != 0xDA, "scan reached"
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise AssertionError(f"no FF {marker:02X} segment")


def _oversubscribed(data: bytes) -> bytes:
    """first DHT table: three codes moved to length 1 (3 codes of 1 bit: more than 2^1), the
    segment length and the number of values unchanged"""
    pos = _segment(data, 0xC4)
    counts = pos + 5  # FF C4, length (2), Tc/Th (1), then the 16 counts
    b = bytearray(data)
    donor = next(i for i in range(15, 0, -1) if b[counts + i] >= 3)
    total = sum(b[counts:counts + 16])
    b[counts + donor] -= 3
    b[counts] += 3
    assert sum(b[counts:counts + 16]) == total and b[counts] > 2
    return bytes(b)


@pytest.fixture(scope="module")
def fixtures():
    return [open(f, "rb").read() for f in FIXTURES[:3]]


def test_oversubscribed_huffman_table(fixtures):
    from rtdm import _lib as L
    from rtdm import jpeg as J
    bad = _oversubscribed(fixtures[0])
    with pytest.raises(L.RtdmError):
        J.entropy_decode(bad)  # from info (table before the frame header) or the decode itself
    plan = J.plan_batch([fixtures[1], bad, fixtures[2]])
    staging, msgs = J.entropy_decode_batch(plan, threads=3)
    assert list(plan.status) == [OK, INVALID, OK]
    for i, d in ((0, fixtures[1]), (2, fixtures[2])):
        coef, qt, inf = J.entropy_decode(d)
        got_c, got_q = J.batch_coefficients(plan, staging, i)
        assert np.array_equal(got_c.numpy(), coef.numpy()) and np.array_equal(got_q.numpy(), qt.numpy()[:inf.ncomp])
    if plan.items[1].nblocks:  # refused by the Huffman stage: it says why
        assert "Huffman" in msgs[1]


def test_dc_symbol_above_15(fixtures):
    """a DC table whose symbol (the bit count of the difference) is 64: refused with the table,
    not fed to the bit reader as a shift count"""
    from rtdm import _lib as L
    from rtdm import jpeg as J
    pos = _segment(fixtures[0], 0xC4)
    assert fixtures[0][pos + 4] == 0x00  # class 0 (DC), table 0
    b = bytearray(fixtures[0])
    b[pos + 5 + 16] = 0x40  # the first value after the 16 counts
    bad = bytes(b)
    with pytest.raises(L.RtdmError):
        J.entropy_decode(bad)
    plan = J.plan_batch([fixtures[1], bad])
    J.entropy_decode_batch(plan)
    assert list(plan.status) == [OK, INVALID]


@pytest.mark.parametrize("selector", [0x40, 0x04])
def test_scan_table_selector_above_3(fixtures, selector):
    from rtdm import _lib as L
    from rtdm import jpeg as J
    pos = _segment(fixtures[0], 0xDA)
    b = bytearray(fixtures[0])
    b[pos + 6] = selector  # FF DA, length (2), Ns (1), component id (1), Td/Ta
    bad = bytes(b)
    with pytest.raises(L.RtdmError):
        J.entropy_decode(bad)
    plan = J.plan_batch([bad, fixtures[1]])
    _, msgs = J.entropy_decode_batch(plan)
    assert list(plan.status) == [INVALID, OK] and msgs[0] and not msgs[1]


def test_440_sampling_is_unsupported():
    from rtdm import jpeg as J
    d422 = dict(variants())["422"]
    pos = _segment(d422, 0xC0)
    luma = pos + 11  # FF C0, length (2), precision (1), height (2), width (2), Nf (1), id (1), H/V
    assert d422[luma] == 0x21 and J.info(d422).supported == 1
    b = bytearray(d422)
    b[luma] = 0x12
    d440 = bytes(b)
    assert J.info(d440).supported == 0
    assert J.supported(d440) is False
    with pytest.raises(NotImplementedError):
        J.entropy_decode(d440)
    plan = J.plan_batch([d440, d422])
    assert list(plan.status) == [UNSUPPORTED, OK] and plan.items[0].nblocks == 0
