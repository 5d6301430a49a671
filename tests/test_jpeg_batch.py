"""CPU: the batched JPEG host stage through the C ABI (rtdm_jpeg_batch_plan,
rtdm_jpeg_entropy_decode_batch): the plan's shared-buffer layout is consistent, and every
image's coefficients and tables equal the single-image rtdm_jpeg_entropy_decode bit for
bit, for every thread count.  The device stage is tests/test_gpu_jpeg_batch.py."""
import numpy as np
import pytest

from jpeg_cases import FIXTURES, progressive, variants

OK, INVALID, UNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def cases():
    return [(f.rsplit("/", 1)[1], open(f, "rb").read()) for f in FIXTURES] + variants()


@pytest.fixture(scope="module")
def singles(cases):
    """the reference: the single-image host stage of every case, computed once"""
    from rtdm import jpeg as J
    out = []
    for _, d in cases:
        coef, qt, inf = J.entropy_decode(d)
        out.append((coef.numpy().copy(), qt.numpy().copy(), inf))
    return out


def _info_tuple(inf):
    return (inf.width, inf.height, inf.ncomp, list(inf.h), list(inf.v), list(inf.bw), list(inf.bh),
            list(inf.coef_off), inf.nblocks, inf.supported)


def _disjoint(ranges, total):
    ranges = sorted(ranges)
    assert all(lo >= 0 and hi > lo for lo, hi in ranges)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
    assert ranges[-1][1] <= total


def test_plan_invariants(cases):
    from rtdm import _lib as L
    from rtdm import jpeg as J
    datas = [d for _, d in cases]
    plan = J.plan_batch(datas)
    lay = plan.layout
    assert lay.n == lay.n_planned == len(datas)
    assert all(s == OK for s in plan.status)
    for d, inf, it in zip(datas, plan.infos, plan.items):
        assert _info_tuple(inf) == _info_tuple(J.info(d))
        assert it.nblocks == inf.nblocks
        assert it.plane_bytes == L.lib().rtdm_jpeg_workspace_bytes(inf)
    _disjoint([(it.block0, it.block0 + it.nblocks) for it in plan.items], lay.nblocks)
    _disjoint([(it.plane_off, it.plane_off + it.plane_bytes) for it in plan.items], lay.workspace_bytes)
    _disjoint([(it.out_off, it.out_off + inf.width * inf.height * 3) for it, inf in zip(plan.items, plan.infos)],
              lay.out_bytes)
    assert len({it.qt_slot for it in plan.items}) == len(datas)
    # [descriptors | qt | coef] in one staging buffer
    assert lay.desc_bytes == L.jpeg_batch_desc_bytes(len(datas)) == plan.desc.size
    assert lay.desc_bytes <= lay.qt_offset and lay.qt_offset + 384 * len(datas) <= lay.coef_offset
    assert lay.coef_offset % 16 == 0 and lay.staging_bytes == lay.coef_offset + lay.nblocks * 128
    assert lay.idct_groups > 0 and lay.color_groups > 0 and lay.uniform == 0


def test_plan_same_size_images_stack(cases):
    from rtdm import jpeg as J
    d = cases[0][1]
    plan = J.plan_batch([d, d, d])
    inf = plan.infos[0]
    assert plan.layout.uniform == 1
    assert [it.out_off for it in plan.items] == [i * inf.width * inf.height * 3 for i in range(3)]
    # caller-provided placement is taken as given; a pitch below 3 * width is refused per image
    plan = J.plan_batch([d, d], out_off=[64, 0], out_pitch=[3 * inf.width + 5, 3 * inf.width - 1])
    assert list(plan.status) == [OK, INVALID] and plan.layout.n_planned == 1
    assert (plan.items[0].out_off, plan.items[0].out_pitch) == (64, 3 * inf.width + 5)
    assert plan.items[1].nblocks == 0


def _check(plan, staging, i, single):
    from rtdm import jpeg as J
    coef, qt = J.batch_coefficients(plan, staging, i)
    rc, rq, inf = single
    assert np.array_equal(coef.numpy(), rc), i
    assert np.array_equal(qt.numpy()[:inf.ncomp], rq[:inf.ncomp]), i


def test_mixed_batch(cases, singles):
    from rtdm import jpeg as J
    plan = J.plan_batch([cases[0][1], progressive(), b"\x00junk", b"\xff\xd8\xff\xd9", cases[3][1]])
    assert list(plan.status) == [OK, UNSUPPORTED, INVALID, INVALID, OK]
    assert [it.nblocks for it in plan.items][1:4] == [0, 0, 0]
    assert plan.layout.n_planned == 2 and plan.layout.nblocks == plan.items[0].nblocks + plan.items[4].nblocks
    staging, msgs = J.entropy_decode_batch(plan)
    assert list(plan.status) == [OK, UNSUPPORTED, INVALID, INVALID, OK] and msgs == [""] * 5
    _check(plan, staging, 0, singles[0])
    _check(plan, staging, 4, singles[3])


@pytest.mark.parametrize("threads", [1, 3, 16, 64, 0])
def test_coefficients_and_tables_match_single(cases, singles, threads):
    """every case in one batch, for each thread count (64 is clamped to 16, 0 = min(n, 16))"""
    import torch
    from rtdm import jpeg as J
    plan = J.plan_batch([d for _, d in cases])
    # a dirty buffer: whatever a batch leaves behind must not depend on what was there
    staging = torch.full((plan.layout.staging_bytes,), 0x5A, dtype=torch.uint8)
    J.entropy_decode_batch(plan, staging, threads=threads)
    assert all(s == OK for s in plan.status)
    for i, single in enumerate(singles):
        _check(plan, staging, i, single)


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_single_image_and_truncated_stream(cases, singles, threads):
    import torch
    from rtdm import jpeg as J
    plan = J.plan_batch([cases[5][1]])
    staging, _ = J.entropy_decode_batch(plan, threads=threads)
    _check(plan, staging, 0, singles[5])
    # a truncated stream decodes to the same zero-filled coefficients as the single call
    d = cases[0][1]
    cut = d[:len(d) // 2]
    plan = J.plan_batch([cases[1][1], cut, cases[2][1]])
    staging = torch.full((plan.layout.staging_bytes,), 0x5A, dtype=torch.uint8)
    J.entropy_decode_batch(plan, staging, threads=threads)
    assert list(plan.status) == [OK, OK, OK]
    coef, qt, inf = J.entropy_decode(cut)
    _check(plan, staging, 1, (coef.numpy(), qt.numpy(), inf))
    _check(plan, staging, 0, singles[1])
    _check(plan, staging, 2, singles[2])


def test_bad_arguments_are_statuses():
    import ctypes
    from rtdm import _lib as L
    from rtdm import jpeg as J
    lib = L.lib()
    lay = L.rtdm_jpeg_batch_layout()
    assert lib.rtdm_jpeg_batch_plan(None, None, 1, None, None, None, None, None, ctypes.byref(lay), None, 0) == INVALID
    d = open(FIXTURES[0], "rb").read()
    plan = J.plan_batch([d])
    small = np.zeros(plan.layout.staging_bytes - 1, np.uint8)
    small[:plan.desc.size] = plan.desc
    st = lib.rtdm_jpeg_entropy_decode_batch(plan.ptrs, plan.lens, 1, plan.items, ctypes.byref(plan.layout),
                                            small.ctypes.data, small.size, 1, plan.status, None, 0)
    assert st == 3  # RTDM_E_CAPACITY
    empty = J.plan_batch([])
    assert empty.layout.n == 0 and empty.layout.nblocks == 0 and empty.layout.idct_groups == 0
